"""CPU-side checks of the GSet op-file writer's ABI: the three symbols, and
ce_core_gset_apply_bound against tests/gset_write_model.py.  No compute calls here."""
import ctypes

import crdtenc
import gset_write_model as wm

INVALID = 64


def test_library_exports_the_writer():
    lib = crdtenc.lib()
    for name in ("ce_core_gset_apply_bound", "ce_core_gset_apply_members_device", "ce_core_gset_apply_members"):
        assert hasattr(lib, name), name
        assert name in crdtenc.EXPORTS
    assert crdtenc.GSET_APPLY_NEW_ONLY == wm.NEW_ONLY and crdtenc.GSET_FILE_MEMBERS == wm.FILE_MEMBERS


def test_bound_is_the_models_worst_case(oracle):
    assert wm.sealed_len(0) == oracle.lib().oc_cryptor_sealed_len(0)
    for n in (0, 1, 223, 224, 4080, 4096, 65535):      # both sides of each bin header's change
        assert wm.sealed_len(n) == oracle.lib().oc_cryptor_sealed_len(n) == crdtenc.sealed_len(n)
    ns = [0, 1, 2, 14, 15, 16, 17, 31, 452, 453, 454, 905, 906, 907, 10000, 453 << 16, (453 << 16) + 1, 1 << 28]
    for pf in (0, 1, 2, 15, 16, 17, 100, 452, 453):
        for n in ns:
            assert crdtenc.gset_apply_bound(n, pf) == (0,) + wm.bound(n, pf), (n, pf)
    # the bound is what the widest members take, file by file
    top = (1 << 64) - 1
    for n, pf in ((0, 5), (7, 5), (16, 16), (33, 16), (907, 0)):
        chunks = wm.cut([top] * n, pf)
        assert wm.bound(n, pf) == (len(chunks), sum(16 + wm.sealed_len(len(wm.clear_text(ch))) for ch in chunks))


def test_bound_refuses_per_file_past_one_page():
    for pf in (454, 455, 1000, 1 << 16, (1 << 32) - 1):
        assert crdtenc.gset_apply_bound(10, pf)[0] == INVALID
    assert crdtenc.gset_apply_bound(1 << 40, 1)[0] == INVALID      # more files than a u32 counts
    # NULL outputs are allowed
    assert crdtenc.lib().ce_core_gset_apply_bound(ctypes.c_uint64(10), ctypes.c_uint32(3), None, None) == 0
