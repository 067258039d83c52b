// Host program of tests/test_specenv_core_cpu.py: bart_amd/csrc/specenv_core.hpp built by a host compiler alone.
//
//   specenv_core_host display IN OUT   IN (doubles): nrows W r stride hassflux rprs, half[r + 1], (hassflux) sflux[W],
//                                      x[nrows][W].  OUT: out[nrows][ceil(W / stride)], specenv::display_row of every
//                                      row: the functions the kernel runs.
//   specenv_core_host reflect IN OUT   IN (doubles): W, then integers i.  OUT (doubles): reflect_index(i, W) of each.
#include <cstdio>
#include <string>
#include <vector>

#include "../bart_amd/csrc/specenv_core.hpp"

using namespace bartrt;

static bool read_all(const char *path, std::vector<double> &v) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(double));
  const bool ok = std::fread(v.data(), sizeof(double), v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

static int write_all(const char *path, const std::vector<double> &v) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return 8;
  const bool ok = std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok ? 0 : 9;
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::vector<double> in;
  if (!read_all(argv[2], in)) return 3;
  if (mode == "display") {
    if (in.size() < 6) return 4;
    const long nrows = (long)in[0], W = (long)in[1], stride = (long)in[3];
    const int r = (int)in[2], hassflux = (int)in[4];
    const double rprs = in[5];
    if (nrows < 1 || W < 1 || r < 0 || r > specenv::kMaxRadius || stride < 1) return 5;
    if (in.size() != 6 + (size_t)(r + 1) + (hassflux ? (size_t)W : 0) + (size_t)nrows * W) return 6;
    // (copies of their own size: the sanitizer sees a read past the end of any of the three)
    const double *p = in.data() + 6;
    const std::vector<double> half(p, p + r + 1);
    p += r + 1;
    const std::vector<double> sflux(p, p + (hassflux ? W : 0));
    p += sflux.size();
    const long Wk = specenv::kept_columns(W, stride);
    std::vector<double> out((size_t)nrows * Wk);
    for (long i = 0; i < nrows; i++) {
      const std::vector<double> x(p + i * W, p + (i + 1) * W);
      specenv::display_row(x.data(), W, hassflux ? sflux.data() : nullptr, rprs, r, half.data(), stride, out.data() + i * Wk);
    }
    return write_all(argv[3], out);
  }
  if (mode == "reflect") {
    if (in.size() < 1 || in[0] < 1) return 4;
    std::vector<double> out;
    for (size_t k = 1; k < in.size(); k++) out.push_back((double)specenv::reflect_index((long)in[k], (long)in[0]));
    return write_all(argv[3], out);
  }
  return 2;
}
