"""The multi-vector entry of the structured M^-1 (nnsdp_solver_apply_minv_structured_multi), host side: needs no GPU."""
import ctypes as C

from nnsdp_amd import _lib


def test_structured_multi_entry_is_exported():
    lib = _lib.load()
    assert any(name == "nnsdp_solver_apply_minv_structured_multi" for name, _, _ in _lib.SYMBOLS)
    fn = lib.nnsdp_solver_apply_minv_structured_multi
    assert fn.restype is C.c_int and len(fn.argtypes) == 5


def test_structured_multi_entry_rejects_null_arguments():
    lib = _lib.load()
    assert lib.nnsdp_solver_apply_minv_structured_multi(None, 1, None, None, None) < 0
    assert b"null" in lib.nnsdp_last_error()
