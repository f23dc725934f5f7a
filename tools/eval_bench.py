#!/usr/bin/env python3
"""Time the text-motion evaluator's get_co_embeddings at reference widths (dim_pose 263, text H 512, motion H 1024,
T = 196, 22 text tokens) with device events, after warm-up; batch 32 (one evaluation batch) and 512.  Also times the GRU
recurrence alone (the motion encoder's 49 steps at B = 32) and reports its rate against the 24 MiB of recurrent weights
each step reads.  Writes one JSON object (stdout and --out).

    timeout -k 10 600 python tools/eval_bench.py [--reps 20] [--out eval_bench.json]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    E = importlib.import_module("motiondiffusion-moe_amd.evaluator")
    L = importlib.import_module("motiondiffusion-moe_amd._lib")
    import evaluator_ref as ER
    ev = E.MotionTextEvaluator()
    st = ER.synth_state({}, 1)
    for k in ("movement_encoder", "text_encoder", "motion_encoder"):
        getattr(ev, k).load_state_dict(st[k])
    ev = ev.cuda().eval()
    res = {"device": torch.cuda.get_device_name(0), "T": 196, "reps": args.reps}
    for B in (32, 512):
        w, p, x = (t.cuda() for t in ER.synth_inputs(B, 196, {}, 2))
        rng = np.random.RandomState(B)
        ml = torch.from_numpy(rng.randint(40, 197, B))
        ml[0] = 196
        cl = torch.from_numpy(rng.randint(3, 23, B))
        med, mn = _time(lambda: ev.get_co_embeddings(w, p, cl, x, ml), args.reps)
        res[f"co_embeddings_B{B}_ms"] = {"median": med, "min": mn}
        med, mn = _time(lambda: ev.get_motion_embeddings(x, ml), args.reps)
        res[f"motion_embeddings_B{B}_ms"] = {"median": med, "min": mn}
    # the recurrence alone: motion encoder, H = 1024, 49 steps, B = 32
    B, T, H = 32, 49, 1024
    pk = ev.motion_encoder.packs()
    gx = torch.randn(B, T, 6 * H, device="cuda") * 0.1
    lh = np.full(B, T, dtype=np.int32)
    ld = torch.from_numpy(lh).cuda()
    lib = L.lib()
    nb = lib.mdm_gru_bidir_workspace_bytes(B, H)
    ws = torch.empty(nb // 4, device="cuda")
    out = torch.empty(B, 2 * H, device="cuda")

    def gru():
        L.check(lib.mdm_gru_bidir(gx.data_ptr(), pk["w_hh"].data_ptr(), pk["b_hh"].data_ptr(), pk["h0"].data_ptr(), ld.data_ptr(),
                                  lh.ctypes.data, B, T, H, out.data_ptr(), ws.data_ptr(), nb, L.stream_ptr()), "mdm_gru_bidir")

    med, mn = _time(gru, args.reps)
    step_us = med * 1000 / T
    wbytes = 2 * 3 * H * H * 4
    res["gru_H1024_B32_49steps_ms"] = {"median": med, "min": mn, "per_step_us": step_us,
                                      "weight_GBps": wbytes / (step_us * 1e-6) / 1e9}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
