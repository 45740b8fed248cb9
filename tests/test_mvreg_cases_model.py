"""CPU checks of the MVReg corpus (tests/mvreg_cases.py), no GPU.

1. Every case has the facts it is built for (a sum past 2^64, a decisive entry at the stated
   position, markers at the block / grid edges, n_blk past 256 or at 1024).
2. The formulation the kernels implement (tests/dotset_model.py mvreg_survivors, and its
   kernel-shaped restatement `rounds` below: 128-bit sums, a dense winner clock that is scattered
   and cleared, an argmax per block and over the block results) equals the sequential oracle on
   every case of A-E.  On F it does NOT: those state files break the antichain precondition of the
   merge form, which is why ce_dotset_host.cpp sends them to the host route.
3. Sensitivity: wrong variants of the PYTHON model (never of a kernel) -- a sum truncated to 64
   bits or clamped there, a reversed tie rule, equal sums taken for equal clocks, a winner clock scattered or
   cleared for its first 256 entries only, an argmax over the first 256 block results or the first
   262,144 candidates only -- each differ from the oracle on named cases of their family: a kernel
   wrong in that way fails those cases.
"""
import pytest

import dotset_model as M
import mvreg_cases as MC
from oracle import crdts as C

CASES = MC.all_cases()
U64 = (1 << 64) - 1


def rounds(cands, later_wins, bug=None):
    """mvreg_survivors (ce_dotset_host.cpp) over k_mv_prep / k_mv_argmax / k_mv_final / k_mv_kill /
    k_mv_clear, statement by statement; `bug` names one wrong variant."""
    n = len(cands)
    clocks = [sorted(c.dots.items()) for c, _ in cands]          # entry order = actor order
    sums = [sum(c for _, c in cl) for cl in clocks]               # (hi, lo) as one integer
    if bug == "sum64":
        sums = [s & U64 for s in sums]
    if bug == "sumsat":      # a sum that clamps at 2^64 - 1 where it should carry
        sums = [min(s, U64) for s in sums]
    alive = [bool(cl) for cl in clocks]
    nb = MC.n_blk(n)
    later = later_wins != (bug == "tie")
    visible = range(n)
    if bug == "grid":        # k_mv_argmax without its grid stride
        visible = range(min(n, nb * MC.K_BLOCK))
    if bug == "final256":    # k_mv_final without its second trip: blocks 256.. are never read
        visible = [i for i in range(n) if (i // MC.K_BLOCK) % nb < MC.K_BLOCK]
    wclock, out = {}, []
    for _ in range(n + 1):   # the host loop: one round per survivor, n + 1 at the most
        best = None
        for i in visible:
            if alive[i]:
                k = (sums[i], i if later else n - 1 - i)
                if best is None or k > best[0]:
                    best = (k, i)
        if best is None:
            break
        w = best[1]
        out.append(w)        # (a winner that did not kill itself wins again and is listed again)
        for e, (a, c) in enumerate(clocks[w]):
            if not (bug == "scatter256" and e >= MC.K_BLOCK):
                wclock[a] = c
        for i in range(n):
            if alive[i] and (all(c <= wclock.get(a, 0) for a, c in clocks[i]) or
                             (bug == "sumkill" and sums[i] == sums[w])):
                alive[i] = False
        for e, (a, _) in enumerate(clocks[w]):
            if not (bug == "clear256" and e >= MC.K_BLOCK):
                wclock[a] = 0
    return [cands[i] for i in sorted(out)]


def run_model(case, survivors):
    """the case through the merge / fold forms of the device route"""
    def fold(reg, lists):
        reg.vals = survivors(reg.vals + [(op[1], op[2]) for ops in lists for op in ops], True)

    def merge(reg, other):
        reg.vals = survivors(reg.vals + other.vals, False)
    return MC.run_steps(case, fold, merge)[1]


_oracle = {}


def oracle_trace(case):
    if case.name not in _oracle:
        _oracle[case.name] = MC.run_oracle(case)[1]
    return _oracle[case.name]


def test_names_unique_and_families_present():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {c.family for c in CASES} == set("ABCDEF")
    assert all(c.purpose and c.target for c in CASES)


def test_no_zero_counters():
    for case in CASES:
        if case.family == "D":
            continue  # counters are 1 + i // 7 and 1 by construction
        for step in case.steps:
            if step[0] == "ops":
                for ops in MC.decode_files(step)[1]:
                    assert all(c > 0 for op in ops or [] for c in op[1].dots.values()), case
            elif step[0] == "states":
                for sw in step[1]:
                    assert all(c > 0 for vc, _ in C.dec_state("mvreg", sw)[1].vals for c in vc.dots.values()), case


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_stated_results(case):
    """what the issue states for a case is what the oracle gives, step return codes included"""
    trace = oracle_trace(case)
    assert [t[0] for t in trace] == (case.rc or [0] * len(case.steps))
    if case.want is not None:
        assert trace[-1][2] == case.want
    if "vals_after_step" in case.facts:
        assert [t[2] for t in trace] == case.facts["vals_after_step"]
    if "statuses" in case.facts:
        assert trace[1][1] == case.facts["statuses"] and trace[1][2] == trace[0][2]


def test_family_a_facts():
    f = {c.name: c.facts["sums"] for c in CASES if c.family == "A"}
    assert sorted(f["A1_dominated_first"]) == [1 << 63, 1 << 64]
    assert sorted(s >> 64 for s in f["A2_dominated_last"]) == [0, 1, 2]
    lo = [s & U64 for s in f["A3_dominated_first"]]
    assert lo[0] == lo[1] == 5 and sorted(s >> 64 for s in f["A3_dominated_first"]) == [0, 1]
    assert f["A4_equal_sums_ab"] == [1 << 64] * 2
    assert [s >> 64 for s in f["A5_dominated_first"]] == [299, 299] and len(set(f["A5_dominated_first"])) == 2
    for name, sums in f.items():   # every case needs the high word
        assert max(sums) > U64, name


def test_family_c_facts():
    for case in (c for c in CASES if c.family == "C"):
        ops = [op for ops in MC.decode_files(case.steps[0])[1] for op in ops]
        W = sorted(ops[0][1].dots)
        k, pos = case.facts["entries"], case.facts["decisive"]
        assert len(W) == k and k > pos
        assert W[pos] in ops[-1][1].dots and not set(W[:pos] + W[pos + 1:]) & set(ops[-1][1].dots)
    assert {(c.facts["entries"], c.facts["decisive"]) for c in CASES if c.family == "C"} == \
        {(256, 255), (257, 256), (513, 512), (513, 255), (513, 256)}


def test_family_d_facts():
    seen = set()
    for case in (c for c in CASES if c.family == "D"):
        n, prefix, marks = case.facts["n"], case.facts["prefix"], case.facts["markers"]
        seen.add((n, prefix))
        ops = [op for run in case.steps[-1][3] for op in run]
        assert len(ops) == n
        single = [i for i, op in enumerate(ops) if min(op[1].dots) >= MC.actor(0, 0xC0)]
        assert single == marks and {0, n - 1} <= set(marks)
        assert case.facts["n_blk"] == min(1024, -(-(n + prefix) // 256))
        if n > 256:
            assert {255, 256} <= set(marks)
        if n > 65536:
            assert case.facts["n_blk"] > 256 and any((m + prefix) // 256 >= 256 for m in marks)
            assert len(case.steps[-1][2]) == 64 and min(case.facts["file_bytes"]) > 4096
            assert len({fa for _, fa, _ in case.steps[-1][2]}) >= 7
        if n > 262144:
            assert case.facts["n_blk"] == 1024 and any(m >= 262144 for m in marks)
        # the chain stays short, so the sequential oracle stays fast
        assert len(oracle_trace(case)[-1][2]) <= len(marks) + 7 + prefix
        assert set(marks) <= set(oracle_trace(case)[-1][2])
    assert seen == {(n, 0) for n in MC.D_SIZES} | {(255, 3), (65536 + 257, 3)}


@pytest.mark.parametrize("case", [c for c in CASES if c.family != "F"], ids=repr)
def test_device_forms_equal_oracle(case):
    want = oracle_trace(case)
    assert run_model(case, M.mvreg_survivors) == want
    assert run_model(case, rounds) == want


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "F"], ids=repr)
def test_irregular_states_break_the_merge_form(case):
    """why the host route exists: the survivor rounds are not MVReg::merge / apply here"""
    want = oracle_trace(case)
    assert run_model(case, M.mvreg_survivors) != want
    assert run_model(case, rounds) != want


SENSITIVE = {
    "sum64": ["A1_dominated_first", "A1_dominated_last", "A2_dominated_first", "A2_dominated_last",
              "A3_dominated_last"],
    "sumsat": ["A5_dominated_last", "A2_dominated_last"],
    "tie": ["B1_op_tie_latest_wins", "B2_state_then_op_ingest", "B2_state_then_op_apply",
            "B3_merge_tie_earliest_wins"],
    "sumkill": ["A4_equal_sums_ab", "A4_equal_sums_ba"],
    "scatter256": ["C1_scatter_k257_pos256", "C1_scatter_k513_pos512", "C1_scatter_k513_pos256"],
    "clear256": ["C2_clear_k257_pos256", "C2_clear_k513_pos512", "C2_clear_k513_pos256"],
    "final256": ["D_n65793", "D_n65793_after_state", "D_n262844"],
    "grid": ["D_n262844"],
}


@pytest.mark.parametrize("bug", sorted(SENSITIVE))
def test_wrong_model_variants_fail_their_cases(bug):
    for name in SENSITIVE[bug]:
        case = MC.by_name(name)
        assert run_model(case, lambda c, lw: rounds(c, lw, bug)) != oracle_trace(case), (bug, name)


def test_entries_below_a_block_do_not_tell():
    """the other side of C's edge: with the decisive entry at position 255 the first-256-only
    variants are still right, so it is position 256 that tells"""
    for bug, name in (("scatter256", "C1_scatter_k256_pos255"), ("clear256", "C2_clear_k256_pos255"),
                      ("clear256", "C2_clear_k513_pos255")):
        case = MC.by_name(name)
        assert run_model(case, lambda c, lw: rounds(c, lw, bug)) == oracle_trace(case), (bug, name)
