"""GPU tests of the Orswot state reader and writer kernels (ce_dotset_io.hip) at their edges,
over the corpus of tests/orswot_state_cases.py (its facts are checked on the CPU by
tests/test_orswot_state_cases_model.py).  Every comparison is byte-exact against
oracle.crdts; the path counts say which route ran."""
import os
import random

import pytest

import crdtenc
import orswot_state_cases as K
from oracle import crdts as C

pytestmark = pytest.mark.gpu
APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
CORE = crdtenc.CORE_VERSION
CASES = K.all_cases()
GUARD = 64
FORMS = {"tile": None, "two_sorts": "CE_SER_TWO_SORTS", "scan": "CE_SER_SCAN_FORM"}


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def names(letters):
    return [c.name for f in letters for c in K.family(f)]


def seal(ctx, key, sws):
    """state files in the format read_remote_states reads, under random nonces"""
    return [CORE + e for e in ctx.encrypt_batch(key, [APP + sw for sw in sws])]


def new_core(ctx, key):
    c = crdtenc.Core(ctx, kind=crdtenc.STATE_ORSWOT, supported=[APP], current_data_version=APP)
    c.set_latest_key(key)
    return c


def routes(core):
    return core.path_count("states_device_read"), core.path_count("states_host_parse")


def want_routes(rs):
    return rs.count("device"), rs.count("host")


def reread_on_host(sw):
    """a written state goes back through the host parser when it has no entry, an entry Dot of an
    actor its clock does not name (F_actor_not_in_clock: neither merge adds one to a clock) or a
    head pattern inside its entries' own bytes (E_spurious_in_*: the writer writes them back)"""
    _, st = C.dec_state("orswot", sw)
    return (not st.entries or any(a not in st.clock.dots for v in st.entries.values() for a in v.dots) or
            K.head_counts(sw)[1] > K.layout(sw)["n"])


def device_bytes(torch, core, want_len, slack=4096):
    buf = torch.full((want_len + slack,), 0xa5, dtype=torch.uint8, device="cuda")
    rc, n = core.state_bytes_device(buf.data_ptr(), buf.numel())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return bytes(buf[:n].cpu().numpy().tobytes())


def writer_check(ctx, torch, key, core, want, forms=("tile",)):
    """host writer, device writer and device compaction of `core` == want, in each form of the
    device writer's bookkeeping; returns the device-written bytes"""
    assert core.state_bytes() == want
    pairs = sum(K.runs_of(want))
    got = None
    for form in forms:
        if FORMS[form]:
            os.environ[FORMS[form]] = "1"
        try:
            before = {p: core.path_count(p) for p in ("compact_device_writer", "ser_entries_scan_form", "ser_entries_tile_form")}
            got = device_bytes(torch, core, len(want))
            assert got == want, form
            f, _ = core.compact_to_buffer(nonce=bytes(24))
            st, pt = ctx.decrypt(key, f[16:])
            assert st == 0 and f[:16] == APP and pt == want, form
            assert core.path_count("compact_device_writer") == before["compact_device_writer"] + 1
            ran = {p: core.path_count(p) - before[p] for p in ("ser_entries_scan_form", "ser_entries_tile_form")}
            assert ran == {"ser_entries_scan_form": 2 * (form == "scan" and pairs > 0),
                           "ser_entries_tile_form": 2 * (form != "scan" and pairs > 0)}, (form, ran)
        finally:
            if FORMS[form]:
                os.environ.pop(FORMS[form], None)
    return got


def ingest_check(ctx, torch, case, forms=("tile",), expect=None, keep=False):
    """The case's files into a fresh core and into the oracle: same return code and statuses, the
    oracle's bytes from the host writer, the device writer and the device compaction, the stated
    routes; the same files under CE_HOST_STATES=1 into a fresh core give the same answers without
    a device read; the device-written bytes, sealed and read by a third core, are read on the
    device (`reread_on_host` says when not) and written back unchanged.
    `expect` replaces the oracle's bytes (family H)."""
    rng = random.Random(len(case.name) * 1000 + len(case.files))
    key = rng.randbytes(32)
    calls = ([[case.facts["primer"]]] if "primer" in case.facts else []) + [case.files]
    core, host, oc = new_core(ctx, key), None, C.Core("orswot")
    os.environ["CE_HOST_STATES"] = "1"
    try:
        host = new_core(ctx, key)
    finally:
        os.environ.pop("CE_HOST_STATES")
    for sws in calls:
        files = seal(ctx, key, sws)
        before = routes(core)
        rc, st = core.ingest_states(files)
        orc, ost = oc.read_remote_states(key, [APP], files)
        assert (rc, st) == (orc, ost) == (0, [0] * len(files)), (rc, st, orc, ost, ctx.last_error())
        got = tuple(a - b for a, b in zip(routes(core), before))
        want_r = want_routes(case.routes) if sws is case.files else (1, 0)
        assert got == want_r, (case.name, got, want_r)
        os.environ["CE_HOST_STATES"] = "1"
        try:
            assert host.ingest_states(files) == (rc, st)
        finally:
            os.environ.pop("CE_HOST_STATES")
    want = oc.serialize() if expect is None else expect
    assert host.state_bytes() == want and host.path_count("states_device_read") == 0
    dev = writer_check(ctx, torch, key, core, want, forms)
    host.close()
    # round trip
    third = new_core(ctx, key)
    assert third.ingest_states(seal(ctx, key, [dev])) == (0, [0])
    assert routes(third) == ((0, 1) if reread_on_host(want) else (1, 0))
    assert third.state_bytes() == want and device_bytes(torch, third, len(want)) == want
    third.close()
    # a file stated `host` beside files stated `device`: alone it is the one the host parses
    if len(set(case.routes)) == 2:
        for sw, r in zip(case.files, case.routes):
            if r == "host":
                one = new_core(ctx, key)
                assert one.ingest_states(seal(ctx, key, [sw])) == (0, [0]) and routes(one) == (0, 1)
                one.close()
    if keep:
        return core, oc, key
    core.close()


# ------------------------------------------------------------------------------------------ A, B, E, F
@pytest.mark.parametrize("name", names("AB"))
def test_widths_and_counts(ctx, torch, name):
    forms = ("tile", "two_sorts", "scan") if name in ("A_cross", "A_wide256", "B_dots_per_entry", "B_entries_65536") else ("tile",)
    ingest_check(ctx, torch, CASES[name], forms)


@pytest.mark.parametrize("name", names("EF"))
def test_reader_edges(ctx, torch, name):
    ingest_check(ctx, torch, CASES[name])


# ------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("name", names("C"))
def test_writer_tiles_and_blocks(ctx, torch, name):
    """each case through the tiled bookkeeping, the two-sort order (CE_SER_TWO_SORTS=1) and the
    head / scan / seg / len / scan form (CE_SER_SCAN_FORM=1); both knobs are read per launch"""
    ingest_check(ctx, torch, CASES[name], ("tile", "two_sorts", "scan"))


# ------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("name", names("D"))
def test_output_placement(ctx, torch, name):
    """state_bytes_device (a) straight into dst = base + k for k in 0..15 with room for the writer's
    bound (head + 5 + 47 x pairs + tail), (b) staged and copied when cap is the exact length, (c)
    INVALID_ARG with the needed length when cap is one short; a5 around and, in (c), inside."""
    case = CASES[name]
    want = case.files[0]
    rng = random.Random(case.facts["residue"])
    key = rng.randbytes(32)
    core = new_core(ctx, key)
    assert core.ingest_states(seal(ctx, key, [want])) == (0, [0]) and routes(core) == (1, 0)
    L = K.layout(want)
    bound = L["prefix"] + 5 + K.SER_MAX_DOT * case.facts["pairs"] + (L["hi"] - L["end"])
    assert bound > len(want)
    buf = torch.empty(GUARD + 16 + bound + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0

    def run(k, cap):
        buf.fill_(0xa5)
        rc, n = core.state_bytes_device(buf.data_ptr() + GUARD + k, cap)
        torch.cuda.synchronize()
        return rc, n, bytes(buf.cpu().numpy().tobytes())
    for k in range(16):
        rc, n, got = run(k, bound)
        assert rc == 0 and n == len(want), (k, rc, n)
        assert got[GUARD + k:GUARD + k + n] == want, k
        assert got[:GUARD + k] == b"\xa5" * (GUARD + k), k
        # (past the clear text the direct branch owns the buffer up to its bound: the 16-byte
        # pieces stay inside [lo, hi), so nothing past the text is written either)
        assert got[GUARD + k + n:] == b"\xa5" * (len(got) - GUARD - k - n), k
    for k in (0, 1, 15):
        rc, n, got = run(k, len(want))
        assert rc == 0 and n == len(want) and got[GUARD + k:GUARD + k + n] == want, k
        assert got[:GUARD + k] == b"\xa5" * (GUARD + k) and got[GUARD + k + n:] == b"\xa5" * (len(got) - GUARD - k - n), k
        rc, n, got = run(k, len(want) - 1)
        assert rc == 64 and n == len(want) and got == b"\xa5" * len(got), k
    core.close()


def test_merge_state_device_at_every_alignment(ctx, torch):
    """the reader's a.s + a.lo at every alignment: one family-A state in HBM at offsets 0..15"""
    sw = CASES["A_cross"].files[0]
    key = bytes(32)
    for k in range(16):
        d = torch.tensor(list(bytes(k) + sw + bytes(32)), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        core = new_core(ctx, key)
        assert core.merge_state_device(d.data_ptr() + k, len(sw)) == 0 and routes(core) == (1, 0), k
        assert core.state_bytes() == sw == device_bytes(torch, core, len(sw)), k
        core.close()


# ------------------------------------------------------------------------------------------ G
@pytest.mark.parametrize("name", names("G"))
def test_many_files(ctx, torch, name):
    """the descriptor batches of 16 and the k-way merge up to 64 files, early (queued behind the
    reader) only when 2..16 files all end in the one canonical empty deferred map; then an op
    batch on top, so a stale scratch word of the call would show"""
    case = CASES[name]
    core, oc, key = ingest_check(ctx, torch, case, keep=True)
    assert core.path_count("states_kway_merge") == int(case.facts["kway"])
    assert core.path_count("states_kway_early") == int(case.facts["early"])
    actors = [K.uid(i, b"ga") for i in range(3)] + [K.uid(0, b"late")]
    ops, fa, fv = [], [], []
    for i, a in enumerate(actors):
        v = oc.nov.get(a)
        base = oc.state.clock.get(a)
        ops.append(C.enc_orswot_ops([("Add", (a, base + 1), [13, 26, 70000 + i]),
                                     ("Rm", C.VClock({a: base + 1, actors[0]: 1}), [13, 39]),
                                     ("Add", (a, base + 2), [39])]))
        fa.append(i)
        fv.append(v)
    files = [CORE + e for e in ctx.encrypt_batch(key, [APP + o for o in ops])]
    rc, st = core.ingest_ops(files, actors, fa, fv)
    assert (rc, st) == oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], fv) == (0, [0] * len(files))
    writer_check(ctx, torch, key, core, oc.serialize())
    core.close()


# ------------------------------------------------------------------------------------------ H
@pytest.mark.parametrize("name", names("H"))
def test_zero_counter_dots(ctx, torch, name):
    """A Dot with counter 0 is no Dot: the device route and the host route give the oracle's bytes
    for the file with its zero-counter Dots removed.  Where the reference (crdts 7, which keeps
    what a file holds) gives the same bytes for the file as it is, that is asserted too; where it
    does not, DESIGN.md lists the departure."""
    case = CASES[name]
    rng = random.Random(7)
    key = rng.randbytes(32)
    strip, ref = C.Core("orswot"), C.Core("orswot")
    assert strip.read_remote_states(key, [APP], seal(ctx, key, [case.facts["stripped"]]))[0] == 0
    assert ref.read_remote_states(key, [APP], seal(ctx, key, case.files))[0] == 0
    assert (ref.serialize() == strip.serialize()) == case.facts["same_as_reference"]
    ingest_check(ctx, torch, case, expect=strip.serialize())
