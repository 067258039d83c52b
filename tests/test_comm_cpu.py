"""CPU: the communicator calls and the block band integration (include/bartrt.h, bartrt_comm_*,
bartrt_step_bandflux_blocks_dev) are declared, exported and bound, and refuse to run without an engine.
Nothing here reaches RCCL (ncclGetUniqueId opens sockets) or the GPU: only the argument checks that run first."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bartrt_comm_get_unique_id", "bartrt_comm_init", "bartrt_comm_free", "bartrt_get_comm",
       "bartrt_step_bandflux_blocks_dev")
EINVAL, ENODEV = -1, -3


@pytest.fixture(scope="module")
def lib():
    from bart_amd import build, transit_module as trm
    build.build()
    return trm.lib()


def _header():
    return open(os.path.join(ROOT, "include", "bartrt.h")).read()


def test_header_declares_the_calls_and_the_id_size():
    txt = _header()
    m = re.search(r"#define\s+BARTRT_COMM_ID_BYTES\s+(\d+)", txt)
    assert m and int(m.group(1)) == 128
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name


def test_the_shim_binds_them(lib):
    from bart_amd import engine
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    assert engine.COMM_ID_BYTES == 128
    for fn in ("comm_init", "comm_attach", "comm_unique_id", "comm_free", "comm_info", "step_bandflux_blocks_dev"):
        assert callable(getattr(engine, fn)), fn


def test_no_engine_is_refused(lib):
    """Without bartrt_init: the engine checks answer before anything reaches RCCL or HIP."""
    uid = (C.c_char * 128)()
    assert lib.bartrt_comm_init(C.cast(uid, C.c_void_p), 0, 1) in (EINVAL, ENODEV)
    assert b"bartrt_init" in lib.bartrt_last_error()
    assert lib.bartrt_comm_free() in (EINVAL, ENODEV)
    r, n, k = C.c_int(7), C.c_int(7), C.c_ulonglong(7)
    assert lib.bartrt_get_comm(C.byref(r), C.byref(n), C.byref(k)) in (EINVAL, ENODEV)
    buf = (C.c_double * 64)()
    st = (C.c_int * 4)()
    band = (C.c_double * 4)()
    assert lib.bartrt_step_bandflux_blocks_dev(C.cast(buf, C.c_void_p), 2, 4, C.cast(st, C.c_void_p),
                                               C.cast(band, C.c_void_p), None) in (EINVAL, ENODEV)
    # a null id buffer is refused before RCCL is looked for
    assert lib.bartrt_comm_get_unique_id(None) == EINVAL
