"""CE_STATE_LWWREG in the C ABI: the header's enumerator, the library's export and the Python
binding's constant.  CPU only (the library is loaded, no device is opened)."""
import os
import re

import crdtenc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "crdtenc.h")) as f:
        return f.read()


def test_header_declares_the_kind():
    h = _header()
    body = re.search(r"enum\s+ce_state_kind\s*\{(.*?)\n\};", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = dict((k, int(v)) for k, v in re.findall(r"(CE_STATE_\w+)\s*=\s*(\d+)", body))
    assert kinds["CE_STATE_LWWREG"] == 6
    assert sorted(kinds.values()) == list(range(7))  # every earlier kind keeps its value


def test_header_declares_the_read():
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+ce_core_lwwreg_read\s*\(\s*ce_core\s*\*\s*c\s*,\s*uint64_t\s*\*\s*val\s*,"
                     r"\s*uint64_t\s*\*\s*marker\s*\)\s*;", h)


def test_library_exports_the_read():
    assert "ce_core_lwwreg_read" in crdtenc.EXPORTS
    assert hasattr(crdtenc.lib(), "ce_core_lwwreg_read")


def test_binding_constant():
    assert crdtenc.STATE_LWWREG == 6
    assert crdtenc.STATE_GSET == 5
