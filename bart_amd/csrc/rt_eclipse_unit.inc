// The ahead-of-time registry of ONE translation unit (rt_launch.hpp), included at the end of each unit that instantiates
// eclipse kernels.  The unit defines
//   BARTRT_UNIT          its name: the object is rt_eclipse_<name>.o
//   BARTRT_UNIT_KERNELS  its kernels, one BARTRT_K(family, template arguments...) each
// and gets find_<name>(id) -- a switch over the ids' keys, so two rows of one id do not compile -- and ids_<name>(&n).
// A row's argument list goes to the family's id maker and to its template alike; naming the template here is what
// instantiates it, in this unit and under this unit's flags.
#define BARTRT_CAT2(a, b) a##b
#define BARTRT_CAT(a, b) BARTRT_CAT2(a, b)

namespace bartrt {

RtKernel BARTRT_CAT(find_, BARTRT_UNIT)(const KernelId &id) {
  switch (kernel_key(id)) {
#define BARTRT_K(family, ...) case kernel_key(family##_id(__VA_ARGS__)): return rt_eclipse_##family<__VA_ARGS__>;
    BARTRT_UNIT_KERNELS
#undef BARTRT_K
    default: return nullptr;
  }
}

const KernelId *BARTRT_CAT(ids_, BARTRT_UNIT)(int *n) {
  static constexpr KernelId ids[] = {
#define BARTRT_K(family, ...) family##_id(__VA_ARGS__),
      BARTRT_UNIT_KERNELS
#undef BARTRT_K
  };
  *n = (int)(sizeof ids / sizeof *ids);
  return ids;
}

}  // namespace bartrt
