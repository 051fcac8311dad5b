"""Generates tests/golden/scenes/*.npz: start scenes in the file format of dgppo.env.Scenes (Scenes.save), from the hand-made scenes
the lookahead tests write in NumPy and one MPESpread pair.  Needs no GPU.
Run from the repo root:  python tests/golden/make_scenes.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import lookahead_np as L  # noqa: E402
import lookahead_rounds_np as R  # noqa: E402
from dgppo_amd.env import scenes as SC  # noqa: E402

OUT = os.path.join(HERE, "scenes")
f32 = np.float32


def from_records(agent, goal, obst):
    """(agent [S, n, 4], goal [S, n, 4], obst [S, no, 16] records) -> the template rows: rect = the records' first five words"""
    return np.asarray(agent, f32), np.asarray(goal, f32), np.ascontiguousarray(obst[..., :5], f32)


def main():
    os.makedirs(OUT, exist_ok=True)
    _, agent, goal, obst = R.scene_a()
    agent, goal, rect = from_records(agent, goal, obst)
    SC.write_npz(os.path.join(OUT, "lidarspread_n2_headon.npz"), "LidarSpread", 2, agent, goal, rect, "rect", ["headon"])
    both = [L.scene(mover)[1:] for mover in (0, 1)]
    agent, goal, rect = from_records(*(np.concatenate([c[k] for c in both]) for k in range(3)))
    SC.write_npz(os.path.join(OUT, "lidarspread_n2_lookahead.npz"), "LidarSpread", 2, agent, goal, rect, "rect",
                 ["mover0", "mover1"])
    # MPESpread, n = 3, two discs (radius 0.05).  swap: agents 0 and 1 fly at each other's goals through the gap between the
    # discs, agent 2 rests aside; wall: agent 0 starts 0.11 from a disc centre (car_radius + obs_radius = 0.1: free by 0.01)
    # and flies at it
    agent = np.array([[[0.3, 0.75, 0.4, 0.0], [1.2, 0.75, -0.4, 0.0], [0.75, 1.3, 0.0, 0.0]],
                      [[0.64, 0.6, 0.5, 0.0], [0.3, 1.2, 0.0, 0.0], [1.2, 1.2, 0.0, 0.0]]], f32)
    goal = np.zeros((2, 3, 4), f32)
    goal[0, :, :2] = [[1.2, 0.75], [0.3, 0.75], [0.75, 0.2]]
    goal[1, :, :2] = [[1.3, 0.6], [0.3, 0.3], [1.2, 0.3]]
    disc = np.array([[[0.75, 0.6], [0.75, 0.9]], [[0.75, 0.6], [0.2, 0.75]]], f32)
    SC.write_npz(os.path.join(OUT, "mpespread_n3_swap_wall.npz"), "MPESpread", 3, agent, goal, disc, "disc", ["swap", "wall"])


if __name__ == "__main__":
    main()
