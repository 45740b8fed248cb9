"""Writes tests/golden/pncounter.json: a handful of Vec<pncounter::Op<Uuid>> blobs and one
StateWrapper<PNCounter<Uuid>> in hex with their decoded forms, packed by Python msgpack alone
(no model code), so the layout is pinned independently of tests/pncounter_model.py's writer.

    python tests/golden/make_pncounter_golden.py
"""
import json
import os

import msgpack

A = [bytes([0x10 * (i + 1)] * 15 + [i]) for i in range(3)]


def op(actor, counter, d):
    return {"dot": {"actor": actor, "counter": counter}, "dir": d}


def pack(x):
    return msgpack.packb(x, use_bin_type=True)


def ops_case(name, ops):
    return {"name": name, "hex": pack([op(*o) for o in ops]).hex(),
            "ops": [[a.hex(), c, d] for a, c, d in ops]}


def vclock(d):
    return {"dots": {a: d[a] for a in sorted(d)}}


def main():
    # one op per counter width: fixint, cc, cd, ce, cf -> 47, 48, 49, 51, 55 bytes
    widths = [5, 200, 0x1234, 0x12345678, 0x123456789abcdef0]
    cases = [ops_case("width_%d" % i, [(A[0], c, "Pos" if i % 2 == 0 else "Neg")]) for i, c in enumerate(widths)]
    cases.append(ops_case("empty", []))
    cases.append(ops_case("mixed", [(A[0], 7, "Pos"), (A[0], 300, "Neg"), (A[1], 1, "Neg"), (A[2], 70000, "Pos"),
                                    (A[1], 1 << 40, "Pos")]))
    nov, p, n = {A[0]: 3, A[2]: 260}, {A[0]: 7, A[2]: 70000}, {A[0]: 300, A[1]: 1}
    state = {"next_op_versions": vclock(nov),
             "state": {"p": {"inner": vclock(p)}, "n": {"inner": vclock(n)}}}
    out = {"op_lengths": [47, 48, 49, 51, 55], "ops": cases,
           "state": {"hex": pack(state).hex(),
                     "next_op_versions": {a.hex(): c for a, c in nov.items()},
                     "p": {a.hex(): c for a, c in p.items()},
                     "n": {a.hex(): c for a, c in n.items()}}}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pncounter.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
