"""BARTRT_SLANT_OPT and bartrt_set_slant_opt / bartrt_get_slant_opt: the guard of the single-wave `cut slant` kernel's
optimistic loop (include/bartrt.h).  No GPU and no engine: the setting is the process's."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_accepts_0_to_10_and_refuses_the_rest():
    from bart_amd import transit_module as trm
    assert trm.parse_slant_opt("0") == 0.0
    for n in range(1, 11):
        assert trm.parse_slant_opt(str(n)) == 2.0 ** -n
    for bad in ("11", "-1", "", "4.0", "four", "4 ", "0x4", "99999999999999999999"):
        with pytest.raises(trm.TransitError):
            trm.parse_slant_opt(bad)


def test_setter_and_getter_round_trip_and_refuse_what_is_no_guard():
    from bart_amd import transit_module as trm
    before = trm.get_slant_opt()
    try:
        for g in [0.0] + [2.0 ** -n for n in range(0, 11)]:
            trm.set_slant_opt(g)
            assert trm.get_slant_opt() == g
        for bad in (2.0, 2.0 ** -11, 0.3, -0.25, float("nan"), float("inf")):
            with pytest.raises(trm.TransitError):
                trm.set_slant_opt(bad)
            assert trm.get_slant_opt() == 2.0 ** -10        # a refused value changes nothing
    finally:
        trm.set_slant_opt(before)


CHILD = """
import sys
sys.path.insert(0, %r)
from bart_amd import transit_module as trm
try:
    print("GUARD %%r" %% trm.get_slant_opt())
except trm.TransitError as e:
    print("REFUSED", e)
    trm.set_slant_opt(0.25)          # the setter names a valid guard: the refusal ends
    print("GUARD %%r" %% trm.get_slant_opt())
""" % ROOT


@pytest.mark.parametrize("value,want", [(None, "GUARD 0.0625"), ("0", "GUARD 0.0"), ("6", "GUARD 0.015625"),
                                        ("11", "REFUSED"), ("on", "REFUSED")])
def test_the_environment_is_read_once_per_process(value, want):
    env = {k: v for k, v in os.environ.items() if k != "BARTRT_SLANT_OPT"}
    if value is not None:
        env["BARTRT_SLANT_OPT"] = value
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith(want), r.stdout
    if want == "REFUSED":
        assert "BARTRT_SLANT_OPT" in lines[0] and lines[1] == "GUARD 0.25", r.stdout
