"""CPU-side checks of the Orswot Rm-op writer's ABI: the two symbols, their names in EXPORTS, the
Core methods and the flag.  No compute calls here."""
import crdtenc


def test_library_exports_the_writer():
    lib = crdtenc.lib()
    for name in ("ce_core_orswot_rm_members_device", "ce_core_orswot_rm_members"):
        assert hasattr(lib, name), name
        assert name in crdtenc.EXPORTS
    for name in ("orswot_rm_members_device", "orswot_rm_members"):
        assert callable(getattr(crdtenc.Core, name))
    assert crdtenc.ORSWOT_RM_LIVE_ONLY == 1
