"""CPU-side checks of tm_fanout_dev_pairs' boundary: the call is exported and
listed, refuses a null handle without touching a device (its other TM_EINVAL
cases need a handle: tests/test_gpu_fanout_pairs.py), and the ABI minor
version moved to 12."""
from emqx_amd import _native, build


def test_the_call_is_exported_and_listed():
    build.build_tmatch()
    lib = _native.load_library()
    assert "tm_fanout_dev_pairs" in _native.EXPORTS and hasattr(lib, "tm_fanout_dev_pairs")
    assert callable(getattr(_native.Index, "fanout_dev_pairs", None))


def test_a_null_handle_is_einval():
    lib = _native.load_library()
    assert lib.tm_fanout_dev_pairs(None, 0, None, None, 0, None, 0, 1, None, None, None, None) == _native.TM_EINVAL
    assert b"null handle" in lib.tm_last_error(None)


def test_abi_minor_version_covers_the_pairs_fanout():
    v = _native.load_library().tm_abi_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 12
