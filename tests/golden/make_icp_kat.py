"""Writes tests/golden/icp_kat.json: one 64-beam point-to-line ICP refine, inputs
and results as hex floats, computed by the restatement (tests/icp_oracle.py).
The vector pins the restatement: tests/test_icp_cpu.py recomputes it.

    python tests/golden/make_icp_kat.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "my-lidar-graph-slam_amd"), os.path.join(ROOT, "tests")]

import icp_oracle as orc  # noqa: E402
from lgs_amd import scene  # noqa: E402


def hx(v):
    return [float(x).hex() for x in v]


def main():
    world = scene.make_world()
    ang = scene.beam_angles(64)
    ref_pose, true = (0.3, -0.2, 0.1), (0.5, 0.0, 0.15)
    ref = orc.ScanIn(scene.ray_cast(world, ref_pose, ang), ang, (0.1, -0.05, 0.02))
    cur = orc.ScanIn(scene.ray_cast(world, true, ang), ang, (-0.03, 0.08, -0.015))
    prm = orc.Params(8, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 3.0)
    ref_robot = orc.move_backward(ref_pose, ref.rel)
    init = orc.move_backward((true[0] + 0.2, true[1] - 0.15, true[2] + 0.05), cur.rel)
    r = orc.refine(prm, ref, ref_robot, cur, init)
    doc = {
        "params": {"num_iterations_max": prm.num_iterations_max, "doubles": hx(prm[1:])},
        "ref": {"ranges": hx(ref.ranges), "angles": hx(ref.angles), "rel": hx(ref.rel), "pose": hx(ref_robot)},
        "scan": {"ranges": hx(cur.ranges), "angles": hx(cur.angles), "rel": hx(cur.rel), "initial_pose": hx(init)},
        "result": {
            "pose_found": r.pose_found, "iterations": r.iterations, "num_pairs": r.num_pairs,
            "initial_pairs": r.initial_pairs, "cost": float(r.cost).hex(), "pair_cost": float(r.pair_cost).hex(),
            "initial_cost": float(r.initial_cost).hex(), "best_sensor_pose": hx(r.best_sensor_pose),
            "estimated_pose": hx(r.estimated_pose), "hessian": hx(r.hessian), "covariance": hx(r.covariance),
            "trajectory": [hx(t) for t in r.trajectory],
        },
    }
    with open(os.path.join(HERE, "icp_kat.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
