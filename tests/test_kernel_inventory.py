"""CPU: bartrt_kernel_inventory (csrc/rt_launch.hpp) is the library.

Every eclipse kernel instantiated ahead of time is one row of one unit's list, and everything the launch needs of it --
the ahead-of-time lookup, the template-id given to the run-time compiler, that compiler's scheduling option -- derives
from the row's id.  Held here against the build's own products: the kernel handles libbartrt.so exports ARE the
inventory's template-ids (an instantiation demangles with every template argument spelled out), each is defined by the
object the inventory names, and the max-ILP flag of a run-time build is the flag bart_amd/build.py gives that object --
but for the two forms csrc/rt_launch.hpp names (rtc_differs_out, rtc_differs_fast_ilp)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = re.compile(r" V void bartrt::(rt_eclipse_\w+<[^>]*>)\(bartrt::RtArgs\)$")

# (molecules, CIA slots) of BARTRT_MC_LIST (csrc/kernels.hpp)
MC = [(m, c) for m in range(1, 7) for c in (0, 1, 2, 4)]
# The forms whose run-time build is not compiled the way their ahead-of-time twin is: built in a max-ILP unit, no max-ILP
# option at run time.  A third one, or one of these gone, is a change of behaviour this test is meant to stop.
RTC_DIFFERS = ({"rt_eclipse_simpson_slant<5, %d, %d, false, 0, false, true>" % mc for mc in MC} |           # tau / intensity outputs
               {"rt_eclipse_fast<5, %d, %d, %s, 0, 1, false, false>" % (*mc, sq) for mc in MC for sq in ("true", "false")})   # rule 0, `cut vertical`


def _nm():
    from bart_amd import build
    hipcc = shutil.which(build._hipcc()) or build._hipcc()
    here = os.path.dirname(os.path.realpath(hipcc))
    for d in (here, os.path.join(here, "..", "lib", "llvm", "bin"), os.path.join(here, "..", "llvm", "bin")):
        if os.path.exists(os.path.join(d, "llvm-nm")):
            return os.path.join(d, "llvm-nm")
    return shutil.which("nm")


def _kernels(nm, path, *flags):
    out = subprocess.run([nm, "-C", *flags, path], capture_output=True, text=True, check=True).stdout
    return {m.group(1) for m in map(KERNEL.search, out.splitlines()) if m}


def test_inventory_is_the_library():
    from bart_amd import build, engine
    build.build()
    nm = _nm()
    if not nm:
        pytest.skip("neither llvm-nm nor nm on this machine")
    inv = engine.kernel_inventory()
    exprs = [e for e, _, _ in inv]
    assert len(exprs) == len(set(exprs)) >= 1000
    in_lib = _kernels(nm, build.LIB, "-D")
    assert set(exprs) == in_lib, (sorted(set(exprs) - in_lib)[:5], sorted(in_lib - set(exprs))[:5])

    # the object of every line defines the line's kernel, and is compiled the way a run-time build would be
    flags = {os.path.splitext(src)[0]: extra for src, extra in build.EXTRA_FLAGS.items()}
    flags.update({name: extra for variants in build.VARIANTS.values() for name, extra in variants})
    by_object = {}
    for e, _, obj in inv:
        by_object.setdefault(obj, set()).add(e)
    for obj, want in by_object.items():
        have = _kernels(nm, os.path.join(build.CSRC, obj + ".o"))
        assert want == have, (obj, sorted(want - have)[:5], sorted(have - want)[:5])
    unit_ilp = lambda obj: "-amdgpu-sched-strategy=max-ilp" in flags.get(obj, [])
    differs = {e for e, ilp, obj in inv if ilp != unit_ilp(obj)}
    assert differs == RTC_DIFFERS, (sorted(differs - RTC_DIFFERS)[:5], sorted(RTC_DIFFERS - differs)[:5])
    assert all(unit_ilp(obj) and not ilp for e, ilp, obj in inv if e in RTC_DIFFERS)


def test_inventory_reports_the_size_it_needs():
    import ctypes as C
    from bart_amd import build, engine, transit_module as trm
    build.build()
    need = sum(len("\t".join((e, "1", o))) + 1 for e, _, o in engine.kernel_inventory()) + 1
    buf = C.create_string_buffer(need - 1)
    assert trm.lib().bartrt_kernel_inventory(buf, need - 1) == -1
    assert str(need) in trm.lib().bartrt_last_error().decode()
    assert trm.lib().bartrt_kernel_inventory(C.create_string_buffer(need), need) == 0
