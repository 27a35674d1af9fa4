"""gklhip_set_small_read_limit: the entry point exists and checks its arguments, which needs no device."""
import ctypes as C


def test_the_setter_exists_and_checks_its_context():
    from gkl_amd import native
    lib = native.load_library()
    assert hasattr(lib, "gklhip_set_small_read_limit")
    for limit in (383, 511, 400):
        assert lib.gklhip_set_small_read_limit(None, C.c_int32(limit)) == native.ERR_INVALID_ARG
        assert "context is NULL" in (lib.gklhip_last_error() or b"").decode()
