#!/usr/bin/env python3
"""Write tests/golden/motion_features.npz by running the REFERENCE's process_file / extract_features.

    python tools/make_motion_features_golden.py REFERENCE_DIR     # the reference checkout's text2motion/ directory

Needs the reference checkout (never available where the GPU tests run).  utils/motion_process.py (and through it
utils/skeleton.py, utils/quaternion.py, utils/paramUtil.py) is imported by path, never copied; the module globals
process_file reads (tgt_offsets, n_raw_offsets, kinematic_chain, face_joint_indx, fid_r, fid_l, l_idx1, l_idx2) are set
here as its __main__ block sets them, and np.float is aliased to float at run time because the reference still uses the
name numpy removed.  Inputs are the seeded synthetic clips of tests/motion_features_ref.py::synth_clip (fp64).  Stored per
case: the input clip, the reference's data and global_positions, the skeleton tables it ran with, the target offsets, and
the smallest relative distance of any squared foot speed from feet_thre (a case under 1e-3 is refused: the exact contact
comparison of the GPU test needs inputs that the reference alone decides clearly).
Cases: t2m with target offsets (120 frames), t2m without (41: uniform_skeleton replaced by the identity), t2m of 2 frames,
KIT with target offsets (60).  Prints e32, the error of the all-fp32 restatement per column group (the GPU test's yardstick),
the round-trip error through the reference's recover_from_ric, and the reference's CPU time per clip."""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_features_ref as MR  # noqa: E402

CASES = (dict(name="t2m_uniform", skel="t2m", n=120, seed=6, tgt_seed=100, feet_thre=0.002),
         dict(name="t2m_plain", skel="t2m", n=41, seed=2, tgt_seed=None, feet_thre=0.002),
         dict(name="t2m_two", skel="t2m", n=2, seed=3, tgt_seed=None, feet_thre=0.002),
         dict(name="kit_uniform", skel="kit", n=60, seed=61, tgt_seed=101, feet_thre=0.05))
MIN_MARGIN = 1e-3


def reference(ref):
    sys.path.insert(0, ref)
    if not hasattr(np, "float"):
        np.float = float  # removed from numpy; the reference still uses the name
    import utils.motion_process as mp
    import utils.paramUtil as pu
    from utils.skeleton import Skeleton
    return mp, pu, Skeleton


def tables(pu, skel):
    if skel == "t2m":
        return dict(chains=pu.t2m_kinematic_chain, raw=pu.t2m_raw_offsets, face=[2, 1, 17, 16], fid_r=[8, 11], fid_l=[7, 10],
                    legs=(5, 8))
    return dict(chains=pu.kit_kinematic_chain, raw=pu.kit_raw_offsets, face=[11, 16, 5, 8], fid_r=[14, 15], fid_l=[19, 20],
                legs=(17, 18))


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/make_motion_features_golden.py REFERENCE_DIR  (the reference's text2motion/ directory)")
    mp, pu, Skeleton = reference(sys.argv[1])
    uniform = mp.uniform_skeleton
    out, meta = {}, {"cases": [], "min_margin": MIN_MARGIN}
    for case in CASES:
        tb = tables(pu, case["skel"])
        sk = MR.skeleton_from_tables(tb["chains"], tb["raw"], tb["face"], tb["fid_l"] + tb["fid_r"], tb["legs"])
        clip = MR.synth_clip(sk, case["n"], case["seed"])
        mp.n_raw_offsets, mp.kinematic_chain = torch.from_numpy(tb["raw"]), tb["chains"]
        mp.face_joint_indx, mp.fid_r, mp.fid_l = tb["face"], tb["fid_r"], tb["fid_l"]
        mp.l_idx1, mp.l_idx2 = tb["legs"]
        tgt = None
        if case["tgt_seed"] is not None:
            pose = MR.synth_clip(sk, 2, case["tgt_seed"])[0]
            tgt = Skeleton(mp.n_raw_offsets, mp.kinematic_chain, "cpu").get_offsets_joints(torch.from_numpy(pose))
            mp.tgt_offsets, mp.uniform_skeleton = tgt, uniform
        else:
            mp.tgt_offsets, mp.uniform_skeleton = None, (lambda positions, target_offset: positions)
        t0 = time.perf_counter()
        data, glob, _, _ = mp.process_file(clip.copy(), case["feet_thre"])
        dt = time.perf_counter() - t0
        again = mp.extract_features(glob.copy(), case["feet_thre"], mp.n_raw_offsets, mp.kinematic_chain, mp.face_joint_indx,
                                    mp.fid_r, mp.fid_l)
        assert np.array_equal(again, data)
        J = sk.J
        tgt_np = None if tgt is None else tgt.numpy()
        # the restatement in the reference's precision mix reproduces it
        d64, g64 = MR.process_file(sk, clip, case["feet_thre"], tgt_np, all32=False)
        assert np.array_equal(g64, glob) and np.array_equal(d64, data), (np.abs(g64 - glob).max(), np.abs(d64 - data).max())
        speed2 = MR.extract_features(sk, glob, case["feet_thre"])[1]
        margin = float(np.abs(speed2.astype(np.float64) - case["feet_thre"]).min() / case["feet_thre"])
        share = float(data[:, -4:].mean())
        if margin < MIN_MARGIN:
            sys.exit(f"case {case['name']}: a squared foot speed lies within {margin:.3g} of feet_thre; choose another seed")
        d32, g32 = MR.process_file(sk, clip, case["feet_thre"], tgt_np, all32=True)
        e32 = {k: float(np.abs(d32[:, s] - data[:, s]).max()) if len(data) else 0.0 for k, s in MR.column_groups(J).items()}
        e32["pos"] = float(np.abs(g32 - glob).max())
        flips = int((d32[:, -4:] != data[:, -4:]).sum())
        rec = mp.recover_from_ric(torch.from_numpy(data).unsqueeze(0).float(), J)[0].numpy()
        rt = float(np.abs(rec - glob[:-1]).max())
        print(f"{case['name']}: data {data.shape} margin {margin:.3g} contact share {share:.2f} fp32 contact flips {flips} "
              f"round trip {rt:.3g} reference {dt * 1e3:.1f} ms\n    e32 " + " ".join(f"{k} {v:.3g}" for k, v in e32.items()))
        n = case["name"]
        out[f"{n}_joints"], out[f"{n}_data"], out[f"{n}_global_positions"] = clip, data, glob
        if tgt_np is not None:
            out[f"{n}_target_offsets"] = tgt_np
        meta["cases"].append(dict(case, margin=margin, contact_share=share, e32=e32, round_trip=rt))
        if f"{case['skel']}_raw_offsets" not in out:
            out[f"{case['skel']}_raw_offsets"] = np.asarray(tb["raw"], np.int64)
            meta[f"{case['skel']}_tables"] = dict(chains=tb["chains"], face=tb["face"], fid_r=tb["fid_r"], fid_l=tb["fid_l"],
                                                  legs=list(tb["legs"]))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "motion_features.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
