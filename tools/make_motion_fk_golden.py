#!/usr/bin/env python3
"""Write tests/golden/motion_fk.npz by running the REFERENCE's process_file and recover_from_rot.

    python tools/make_motion_fk_golden.py REFERENCE_DIR     # the reference checkout's text2motion/ directory

Needs the reference checkout (never available where the GPU tests run); its modules are imported by path, never copied, as
tools/make_motion_features_golden.py does.  Per skeleton (t2m, KIT) a batch of B = 3 motions in T = 24 frames with lengths
24, 2, 1: rows from the reference's process_file of the seeded clips of tests/motion_features_ref.py::synth_clip ("clean"),
and the same rows with gaussian noise on ALL columns ("noisy": the rot6d pairs are not orthonormal, as a network's are not,
and the position columns no longer agree with them).  The noise scale is chosen so that every rot6d pair keeps |x_raw| >=
MIN_NORM and |x_raw x y_raw| >= MIN_NORM: that bounds the conditioning of cont6d_to_matrix's Gram-Schmidt step, without
which a tolerance means nothing; the generator asserts it.  Rows are stored normalised, (data - mean) / std in fp32, with
the mean / std; every consumer de-normalises them in fp32, rows * std + mean, which is what the reference is handed here.
Stored per case, valid frames only (samples concatenated): the reference's recover_from_rot joints (fp32) on shared offsets
(get_offsets_joints of sample 0's first frame); the fp64 restatement's joints and global rotations on those offsets, and its
mean-bone-length offsets; in ``meta`` the yardsticks: the error of the reference's fp32 joints, of the fp32 restatement's
rotations and of its mean-bone-length offsets against the fp64 restatement, and the distance of the fp32 restatement from
the reference."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import motion_features_ref as MR  # noqa: E402
import motion_fk_ref as FR  # noqa: E402
from make_motion_features_golden import reference, tables  # noqa: E402

T, LENGTHS = 24, (24, 2, 1)
SKELS = (dict(skel="t2m", seed=20, feet_thre=0.002), dict(skel="kit", seed=30, feet_thre=0.05))
NOISE, MIN_NORM = 0.1, 0.2


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/make_motion_fk_golden.py REFERENCE_DIR  (the reference's text2motion/ directory)")
    mp, pu, Skeleton = reference(sys.argv[1])
    out, meta = {}, {"cases": [], "T": T, "lengths": list(LENGTHS), "noise": NOISE, "min_norm": MIN_NORM}
    for spec in SKELS:
        tb = tables(pu, spec["skel"])
        sk = MR.skeleton_from_tables(tb["chains"], tb["raw"], tb["face"], tb["fid_l"] + tb["fid_r"], tb["legs"])
        F = 12 * sk.J - 1
        mp.n_raw_offsets, mp.kinematic_chain = torch.from_numpy(tb["raw"]), tb["chains"]
        mp.face_joint_indx, mp.fid_r, mp.fid_l = tb["face"], tb["fid_r"], tb["fid_l"]
        mp.l_idx1, mp.l_idx2 = tb["legs"]
        mp.tgt_offsets, mp.uniform_skeleton = None, (lambda positions, target_offset: positions)
        clean, first = [], None
        for i, n in enumerate(LENGTHS):
            data, glob, _, _ = mp.process_file(MR.synth_clip(sk, n + 1, spec["seed"] + i), spec["feet_thre"])
            clean.append(data.astype(np.float32))
            first = glob[0] if first is None else first
        skel = Skeleton(mp.n_raw_offsets, mp.kinematic_chain, "cpu")
        offsets = skel.get_offsets_joints(torch.from_numpy(first).float()).numpy()
        rng = np.random.RandomState(spec["seed"])
        mean, std = (0.1 * rng.randn(F)).astype(np.float32), (0.5 + rng.rand(F)).astype(np.float32)
        out[f"{spec['skel']}_offsets"], out[f"{spec['skel']}_mean"], out[f"{spec['skel']}_std"] = offsets, mean, std
        for kind in ("clean", "noisy"):
            name = f"{spec['skel']}_{kind}"
            rows = np.zeros((len(LENGTHS), T, F), np.float32)
            for i, d in enumerate(clean):
                d = d + (NOISE * rng.randn(*d.shape)).astype(np.float32) if kind == "noisy" else d
                rows[i, :len(d)] = (d - mean) / std
            ref, j64, r64, o64, margins = [], [], [], [], []
            e = dict(joints=0.0, rotations=0.0, offsets=0.0, restatement=0.0)
            for i, n in enumerate(LENGTHS):
                data = rows[i, :n] * std + mean  # fp32: what every consumer computes
                margins.append(FR.gram_schmidt_margins(sk, data))
                got = mp.recover_from_rot(torch.from_numpy(data).float(), sk.J, skel).numpy()
                a64, b64 = FR.recover_from_rot(sk, data, offsets, torch.float64, return_rotations=True)
                a32, b32 = FR.recover_from_rot(sk, data, offsets, torch.float32, return_rotations=True)
                m64, m32 = FR.mean_bone_offsets(sk, data, torch.float64), FR.mean_bone_offsets(sk, data, torch.float32)
                e["joints"] = max(e["joints"], float(np.abs(got - a64).max()))
                e["rotations"] = max(e["rotations"], float(np.abs(b32 - b64).max()))
                e["offsets"] = max(e["offsets"], float(np.abs(m32 - m64).max()))
                e["restatement"] = max(e["restatement"], float(np.abs(a32 - got).max()))
                ref.append(got), j64.append(a64), r64.append(b64), o64.append(m64)
            lo = (min(m[0] for m in margins), min(m[1] for m in margins))
            assert min(lo) >= MIN_NORM, f"{name}: |x_raw| >= {lo[0]:.3g}, |x_raw x y_raw| >= {lo[1]:.3g}: lower NOISE"
            print(f"{name}: |x_raw| >= {lo[0]:.3g} |x x y_raw| >= {lo[1]:.3g}  " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
            out[f"{name}_rows"], out[f"{name}_ref_joints"] = rows, np.concatenate(ref)
            out[f"{name}_joints64"], out[f"{name}_rotations64"] = np.concatenate(j64), np.concatenate(r64)
            out[f"{name}_offsets64"] = np.stack(o64)
            meta["cases"].append(dict(name=name, skel=spec["skel"], kind=kind, min_x=lo[0], min_cross=lo[1], yardstick=e))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "motion_fk.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
