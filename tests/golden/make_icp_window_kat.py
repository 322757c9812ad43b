"""Writes tests/golden/icp_window_kat.json: the window search of a 16-beam scan
against three 16-beam reference scans over a 3 x 3 x 3 lattice -- the lattice
poses, every pose's cost and pairs, the best index, the refine from the best
pose, the gate's terms and answer and the 176-byte record -- inputs and results
as hex floats, computed by the restatement (tests/icp_window_oracle.py over
tests/icp_ref_oracle.py).  The vector pins the restatement:
tests/test_icp_window_cpu.py recomputes it.

    python tests/golden/make_icp_window_kat.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "my-lidar-graph-slam_amd"), os.path.join(ROOT, "tests")]

import icp_oracle as orc  # noqa: E402
import icp_ref_oracle as rorc  # noqa: E402
import icp_window_oracle as worc  # noqa: E402
from lgs_amd import scene  # noqa: E402


def hx(v):
    return [float(x).hex() for x in v]


def compute(doc=None):
    """the vector's inputs (made from the scene when doc is None, else read from doc) and its results"""
    if doc is None:
        world = scene.make_world()
        ang = scene.beam_angles(16)
        rel = (0.1, -0.05, 0.02)
        sensors = [(0.1 * k - 0.1, 0.05 * k - 0.05, 0.02 * k) for k in range(3)]
        refs = [orc.ScanIn(scene.ray_cast(world, s, ang), ang, rel) for s in sensors]
        poses = [orc.move_backward(s, rel) for s in sensors]
        true = (0.05, 0.02, 0.03)
        cur = orc.ScanIn(scene.ray_cast(world, true, ang), ang, (-0.03, 0.08, -0.015))
        prm = orc.Params(4, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 3.0)
        centre = orc.move_backward((true[0] + 0.1, true[1] - 0.08, true[2] + 0.03), cur.rel)
        window = worc.Window(1, 1, 1, 0.1, 0.03)
        gate = worc.Gate(5, 1.0, 0.3, 0.2)
        node = {"pose": (-0.2, 0.1, 0.05), "index": 7, "end_index": 31}
        doc = {
            "params": {"num_iterations_max": prm.num_iterations_max, "doubles": hx(prm[1:])},
            "refs": [{"ranges": hx(s.ranges), "angles": hx(s.angles), "rel": hx(s.rel), "pose": hx(p)}
                     for s, p in zip(refs, poses)],
            "scan": {"ranges": hx(cur.ranges), "angles": hx(cur.angles), "rel": hx(cur.rel), "centre": hx(centre)},
            "window": {"halves": list(window[:3]), "steps": hx(window[3:])},
            "gate": {"min_pairs": gate.min_pairs, "doubles": hx(gate[1:])},
            "node": {"pose": hx(node["pose"]), "index": node["index"], "end_index": node["end_index"]},
        }
    un = lambda v: [float.fromhex(x) for x in v]
    prm = orc.Params(doc["params"]["num_iterations_max"], *un(doc["params"]["doubles"]))
    refs = [orc.ScanIn(un(r["ranges"]), un(r["angles"]), tuple(un(r["rel"]))) for r in doc["refs"]]
    poses = [tuple(un(r["pose"])) for r in doc["refs"]]
    cur = orc.ScanIn(un(doc["scan"]["ranges"]), un(doc["scan"]["angles"]), tuple(un(doc["scan"]["rel"])))
    centre = tuple(un(doc["scan"]["centre"]))
    window = worc.Window(*doc["window"]["halves"], *un(doc["window"]["steps"]))
    gate = worc.Gate(doc["gate"]["min_pairs"], *un(doc["gate"]["doubles"]))
    node_pose = tuple(un(doc["node"]["pose"]))

    rt = rorc.concat_tables(prm, refs, poses)
    cost, pairs = worc.scores(prm, rt.table, cur, centre, window)
    best = worc.select(cost)
    start = worc.lattice_pose(window, centre, best)
    r = rorc.refine(prm, refs, poses, cur, start, rt)
    terms = worc.gate_terms(r, start)
    accepted = worc.gate_accepts(gate, r, start)
    rec = worc.record(node_pose, doc["node"]["index"], doc["node"]["end_index"], r, accepted, len(cur.ranges))
    # the same refine under a gate it cannot pass, and a candidate without a winner
    tight = worc.Gate(gate.min_pairs, gate.max_normalized_cost, 0.0, gate.max_rotation)
    rec_rejected = worc.record(node_pose, doc["node"]["index"], doc["node"]["end_index"], r,
                               worc.gate_accepts(tight, r, start), len(cur.ranges))
    rec_none = worc.record(node_pose, doc["node"]["index"], doc["node"]["end_index"], None, False, len(cur.ranges))
    result = {
        "poses": [hx(worc.lattice_pose(window, centre, p)) for p in range(worc.num_poses(window))],
        "cost": hx(cost), "pairs": [int(v) for v in pairs], "best": best,
        "refine": {"pose_found": r.pose_found, "iterations": r.iterations, "num_pairs": r.num_pairs,
                   "initial_pairs": r.initial_pairs, "initial_cost": float(r.initial_cost).hex(),
                   "normalized_cost": float(r.normalized_cost).hex(), "estimated_pose": hx(r.estimated_pose),
                   "covariance": hx(r.covariance)},
        "gate_terms": [terms[0]] + hx(terms[1:]), "accepted": bool(accepted),
        "record": rec.hex(), "record_rejected": rec_rejected.hex(), "record_none": rec_none.hex(),
    }
    return doc, result


def main():
    doc, result = compute()
    doc["result"] = result
    with open(os.path.join(HERE, "icp_window_kat.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
