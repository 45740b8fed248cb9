"""Writes tests/golden/lwwreg.json: Vec<LWWReg<u64, u64>> op bodies and StateWrapper<LWWReg>
states in hex with their decoded forms, packed by Python msgpack alone (no model code), so the
layout is pinned independently of tests/lwwreg_model.py's writer.

    python tests/golden/make_lwwreg_golden.py
"""
import json
import os

import msgpack

A = [bytes([0x10 * (i + 1)] * 15 + [i]) for i in range(3)]
# both sides of every width boundary, and the largest value
EDGES = [0, 1, 0x7f, 0x80, 0xff, 0x100, 0xffff, 0x10000, (1 << 32) - 1, 1 << 32, (1 << 63), (1 << 64) - 1]
WIDTH = {0: 1, 1: 1, 0x7f: 1, 0x80: 2, 0xff: 2, 0x100: 3, 0xffff: 3, 0x10000: 5, (1 << 32) - 1: 5,
         1 << 32: 9, 1 << 63: 9, (1 << 64) - 1: 9}


def pack(x):
    return msgpack.packb(x, use_bin_type=True)


def reg(val, marker):
    return {"val": val, "marker": marker}  # (dict order is the packed key order)


def ops_case(name, ops, raw=None):
    b = raw if raw is not None else pack([reg(v, m) for v, m in ops])
    return {"name": name, "hex": b.hex(), "ops": [list(o) for o in ops]}


def state_case(name, nov, val, marker):
    sw = {"next_op_versions": {"dots": {a: nov[a] for a in sorted(nov)}}, "state": reg(val, marker)}
    return {"name": name, "hex": pack(sw).hex(), "next_op_versions": {a.hex(): c for a, c in nov.items()},
            "val": val, "marker": marker}


def main():
    ops = [ops_case("empty", []),
           ops_case("val_edges", [(v, 5) for v in EDGES]),
           ops_case("marker_edges", [(5, m) for m in EDGES]),
           ops_case("both_edges", [(v, m) for v in EDGES[::3] for m in EDGES[::3]]),
           ops_case("fifteen", [((1 << 33) + i, 0x100 + i) for i in range(15)]),   # 9f: the last fixarray
           ops_case("sixteen", [((1 << 33) + i, 0x100 + i) for i in range(16)])]   # dc 00 10
    for i, e in enumerate(EDGES):
        ops.append(ops_case("one_val_%d" % i, [(e, 1)]))
        ops.append(ops_case("one_marker_%d" % i, [(1, e)]))
    # forms from_slice also takes: the struct as an array, and the keys the other way round
    ops.append(ops_case("array_form", [(7, 0x1234), (1 << 40, 9)], pack([[7, 0x1234], [1 << 40, 9]])))
    ops.append(ops_case("reversed_keys", [(7, 0x1234), (1 << 40, 9)],
                        pack([{"marker": 0x1234, "val": 7}, {"marker": 9, "val": 1 << 40}])))
    states = [state_case("default", {}, 0, 0)]
    for i, e in enumerate(EDGES):
        states.append(state_case("val_%d" % i, {A[0]: 3}, e, 0x1234))
        states.append(state_case("marker_%d" % i, {A[1]: 1, A[2]: 260}, 0x1234, e))
    out = {"element_lengths": {hex(v): 12 + WIDTH[v] + 1 for v in EDGES}, "ops": ops, "states": states}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lwwreg.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
