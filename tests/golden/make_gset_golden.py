"""Writes tests/golden/gset.json: Vec<u64> op bodies and StateWrapper<GSet<u64>> states in hex
with their decoded forms, packed by Python msgpack alone (no model code), so the layout is pinned
independently of tests/gset_model.py's writer.

The two cases past the 16-bit array header (65,535 / 65,536 members) would be most of a megabyte
in hex: they are recorded as their rule (member i = i & 0x7f, so one byte each), header bytes,
length and SHA-256.

    python tests/golden/make_gset_golden.py
"""
import hashlib
import json
import os

import msgpack

A = [bytes([0x10 * (i + 1)] * 15 + [i]) for i in range(3)]
# both sides of every width boundary, and the largest member
EDGES = [0, 1, 0x7f, 0x80, 0xff, 0x100, 0xffff, 0x10000, (1 << 32) - 1, 1 << 32, (1 << 63), (1 << 64) - 2,
         (1 << 64) - 1]


def pack(x):
    return msgpack.packb(x, use_bin_type=True)


def ops_case(name, members):
    return {"name": name, "hex": pack(members).hex(), "members": members}


def big_case(n):
    b = pack([i & 0x7f for i in range(n)])
    return {"count": n, "head": b[:5].hex(), "len": len(b), "sha256": hashlib.sha256(b).hexdigest()}


def state_case(name, nov, members):
    """members as written: ascending (BTreeSet order)"""
    sw = {"next_op_versions": {"dots": {a: nov[a] for a in sorted(nov)}}, "state": {"value": sorted(members)}}
    return {"name": name, "hex": pack(sw).hex(), "next_op_versions": {a.hex(): c for a, c in nov.items()},
            "members": sorted(members)}


def main():
    ops = [ops_case("empty", []), ops_case("edges", EDGES), ops_case("edges_reversed", EDGES[::-1]),
           ops_case("repeated", [7, 7, 1 << 40, 7, 1 << 40]),
           ops_case("fifteen", [(1 << 33) + i for i in range(15)]),   # 9f: the last fixarray
           ops_case("sixteen", [(1 << 33) + i for i in range(16)])]   # dc 00 10: the first array 16
    for i, m in enumerate(EDGES):
        ops.append(ops_case("one_%d" % i, [m]))
    states = [state_case("empty", {}, []), state_case("edges", {A[0]: 3, A[2]: 260}, EDGES),
              state_case("fifteen", {A[1]: 1}, [0x100 + i for i in range(15)]),
              state_case("sixteen", {A[1]: 1}, [0x100 + i for i in range(16)])]
    out = {"element_lengths": {"0x7f": 1, "0x80": 2, "0xff": 2, "0x100": 3, "0xffff": 3, "0x10000": 5,
                               "0xffffffff": 5, "0x100000000": 9, "0xffffffffffffffff": 9},
           "ops": ops, "ops_big": [big_case(65535), big_case(65536)], "states": states}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gset.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
