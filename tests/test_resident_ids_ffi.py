"""The C entry that reads a device-parsed batch's resident ids back is declared, bound and exported."""
import ctypes as C
import os
import re

from snapgpu import _ffi

NAME = "snapgpu_device_reads_ids_download"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ffi_binds_ids_download():
    assert NAME in _ffi.EXPORTED_SYMBOLS
    (res, args), = [(r, a) for n, r, a in _ffi._PROTOS if n == NAME]
    assert res is C.c_int and len(args) == 9
    assert args[3] is C.c_uint64 and args[4] == C.POINTER(C.c_uint64)
    fn = getattr(_ffi.lib(), NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == list(args)


def test_header_declares_ids_download():
    header = open(os.path.join(ROOT, "include", "snapgpu.h")).read()
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == 9


def test_run_sam_and_run_bam_default_to_the_resident_state():
    import inspect

    import snapgpu
    for fn in (snapgpu.DeviceReads.run_sam, snapgpu.DeviceReads.run_bam):
        assert inspect.signature(fn).parameters["reads"].default is None
    assert callable(snapgpu.DeviceReads.ids)
