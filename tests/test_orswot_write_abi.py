"""CPU-side checks of the Orswot add-op writer's ABI: the three symbols, and
ce_core_orswot_add_bound against tests/orswot_write_model.py.  No compute calls here."""
import ctypes

import crdtenc
import orswot_write_model as wm

INVALID = 64


def test_library_exports_the_writer():
    lib = crdtenc.lib()
    for name in ("ce_core_orswot_add_bound", "ce_core_orswot_add_members_device", "ce_core_orswot_add_members"):
        assert hasattr(lib, name), name
        assert name in crdtenc.EXPORTS
    for name in ("orswot_add_members_device", "orswot_add_members"):
        assert callable(getattr(crdtenc.Core, name))


def test_bound_is_the_models_worst_case():
    ns = [0, 1, 2, 14, 15, 16, 17, 27, 28, 29, 57, 58, 59, 445, 446, 447, 892, 893, 10000, 1 << 20, (1 << 32) - 1,
          1 << 32, 1 << 36]
    pairs = [(0, 0), (1, 0), (1, 1), (1, 15), (1, 16), (1, 17), (1, 28), (1, 29), (1, 58), (2, 0), (5, 7), (15, 1),
             (16, 1), (17, 1), (16, 0), (17, 0), (100, 0), (223, 1), (446, 1), (446, 0)]
    for po, k in pairs:
        for n in ns:
            want = wm.bound(n, po, k)
            if want[1] >= 1 << 32:      # max_files is a u32
                assert crdtenc.orswot_add_bound(n, po, k)[0] == INVALID, (n, po, k)
            else:
                assert crdtenc.orswot_add_bound(n, po, k) == (0,) + want, (n, po, k)


def test_bound_refuses_pairs_past_one_page():
    for po, k in ((1, 59), (1, 1 << 16), (447, 1), (447, 0), (446, 2), (5, 39), (16, 20), (1 << 20, 0),
                  ((1 << 32) - 1, (1 << 32) - 1), (1, (1 << 32) - 1)):
        assert wm.shape(po, k) is None
        assert crdtenc.orswot_add_bound(10, po, k)[0] == INVALID, (po, k)
    assert wm.shape(5, 38) == (5, 38) and crdtenc.orswot_add_bound(10, 5, 38)[0] == 0
    assert wm.shape(16, 19) == (16, 19) and crdtenc.orswot_add_bound(10, 16, 19)[0] == 0
    assert crdtenc.orswot_add_bound(1 << 40, 1, 1)[0] == INVALID     # more files than a u32 counts
    # NULL outputs are allowed
    assert crdtenc.lib().ce_core_orswot_add_bound(ctypes.c_uint64(10), ctypes.c_uint32(3), ctypes.c_uint32(0), None,
                                                  None, None) == 0
