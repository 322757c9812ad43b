"""Writes tests/golden/loop_search_kat.json: the nearest-node loop search of
ten hints over a 40-node, 5-map snapshot, inputs and results as hex floats,
computed by the restatement (tests/loop_search_oracle.py).  The poses lie on a
lattice whose steps are (3, 4) or (4, 3) times a power of two, so every hypot
of the travel chain is exact and the file does not depend on the libm build.
The vector pins the restatement: tests/test_loop_search_cpu.py recomputes it.

    python tests/golden/make_loop_search_kat.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "my-lidar-graph-slam_amd"), os.path.join(ROOT, "tests")]

import loop_search_cases as lc  # noqa: E402
import loop_search_oracle as orc  # noqa: E402


def hx(v):
    return [float(x).hex() for x in v]


def main():
    poses = lc.lattice_path(40, 11)
    lo, hi = lc.ranges_of([8, 1, 12, 9, 10])
    acc = lc.accum_at(poses)
    prm = orc.Params(6.0, 20.0, 2)
    hints = lc.hints_of_nodes(range(30, 40, 2), lo, hi, acc)
    hints += lc.hints_of_nodes([21, 25, 29], lo, hi, acc)            # a finished map's nodes as the latest
    hints += [orc.Hint(39, 4, 5, 0.0), orc.Hint(39, 4, 3, acc[39])]   # cut at 0; fewer maps
    travel = orc.travel_chain(poses, lo, hi)
    res, tab = orc.search_all(poses, lo, hi, prm, hints, own_chain=True)
    doc = {
        "poses": [hx(p) for p in poses],
        "idx_min": lo, "idx_max": hi,
        "params": {"travel_dist_threshold": float(prm[0]).hex(), "node_dist_threshold": float(prm[1]).hex(),
                   "num_candidate_nodes": prm[2]},
        "hints": [[h[0], h[1], h[2], float(h[3]).hex()] for h in hints],
        "travel": hx(travel),
        "accum_travel_dist": float(orc.accum_travel_dist(poses)).hex(),
        "records": [[int(v) for v in list(r)[:6]] + [float(r["dist_sq"]).hex()] for r in res],
        "per_map": [[[int(e["node_idx"]), float(e["dist_sq"]).hex()] for e in row] for row in tab],
    }
    with open(os.path.join(HERE, "loop_search_kat.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
