"""The forced-rerun shapes of tests/test_gpu_nif_chain.py, checked with no GPU:
each case's totals (total before aggre/1, K after, T deliveries, G distinct
subscribers) come from the oracle and the tables in plain numpy
(tests/nif_chain_shapes.py) and must stand to a fresh set's first capacities as
the case needs.  The capacities are not restated: the seven c_src units and the
GPU tests' shim (tests/native/nif_chain_shim.c) are linked against the stand-in
libtmatch, and shim_ids_per_topic / shim_first_cap -- TMN_IDS_PER_TOPIC and
tmn_get's growth rule themselves -- give them.
"""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

from nif_chain import UNITS
from nif_chain_shapes import CASES, check_case

ROOT = Path(__file__).resolve().parent.parent
NATIVE = ROOT / "tests" / "native"
FAKES = ("", "_route", "_aggre", "_dispatch", "_share", "_deliver", "_publish_deliver")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("nifshapes") / "libnifshapes.so"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}", "-o", str(out)]
                   + [str(ROOT / "c_src" / f"tmatch_nif_{u}.c") for u in UNITS]
                   + [str(NATIVE / f"fake_tmatch{u}.c") for u in FAKES] + [str(NATIVE / "nif_chain_shim.c")], check=True)
    lib = C.CDLL(str(out))
    lib.shim_ids_per_topic.restype = C.c_uint32
    lib.shim_first_cap.argtypes, lib.shim_first_cap.restype = [C.c_void_p, C.c_uint64], C.c_uint64
    return lib


def test_the_constant_is_the_headers(shim):
    header = (ROOT / "c_src" / "tmatch_nif_core.h").read_text()
    assert f"#define TMN_IDS_PER_TOPIC {shim.shim_ids_per_topic()} " in header


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_shape_forces_the_rerun_it_is_meant_to(shim, case):
    p = check_case(case, shim.shim_ids_per_topic(), lambda words: shim.shim_first_cap(C.c_void_p(1), words))
    print(f"{case}: {p}")
    assert p["cap"] > 0 and p["pd_dcap"] > p["cap"]
