#!/usr/bin/env python3
"""Write tests/golden/evaluator.npz by running the REFERENCE's evaluator networks and metric functions.

    python tools/make_evaluator_golden.py REFERENCE_DIR     # the reference checkout's text2motion/ directory

Needs the reference checkout (never available where the GPU tests run).  datasets1/evaluator_models.py, utils/metrics.py
and datasets1/evaluator.py are imported by file path (the datasets1 package pulls in the dataset stack; the wrapper's
module only needs ``models`` stubbed), never copied.  Weights and inputs are the seeded ones of tests/evaluator_ref.py;
only outputs are stored:
  (a) reduced widths (text H 32, motion H 48, latent 64, dim_pose 263), B = 6, T = 40, ragged unsorted m_lens:
      the wrapper's get_co_embeddings (text / motion embeddings, align order) and the movements
  (b) reference widths, B = 4, T = 196: embeddings only
  (c) metrics on seeded embedding sets: matching score and R-precision counts, FID (N > D), diversity and multimodality
      under np.random.seed
  (d) the reference modules' state-dict keys and shapes at default widths."""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import evaluator_ref as ER  # noqa: E402

CASE_A = dict(B=6, T=40, seed=11, m_lens=[40, 17, 33, 8, 25, 12], cap_lens=[22, 15, 12, 9, 5, 3],
              dims=dict(dim_text_hidden=32, dim_motion_hidden=48, dim_movement_enc_hidden=64, dim_movement_latent=64,
                        dim_coemb_hidden=64))
CASE_A2 = dict(B=6, T=40, seed=12, m_lens=[21, 40, 9, 36, 16, 28], cap_lens=[20, 20, 14, 9, 9, 4],
               dims=dict(dim_text_hidden=48, dim_motion_hidden=32, dim_movement_enc_hidden=64, dim_movement_latent=64,
                         dim_coemb_hidden=64))
CASE_B = dict(B=4, T=196, seed=21, m_lens=[120, 196, 64, 152], cap_lens=[22, 17, 12, 6], dims={})
METRICS = dict(seed=31, n_pairs=96, batch_size=32, n_gt=700, n_gen=650, n_div=400, div_times=300, mm=(8, 12), mm_times=10,
               div_seed=5, mm_seed=6)


def _load(name, path, package=None):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    if package:
        mod.__package__ = package
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference(ref):
    sys.path.insert(0, ref)  # utils.* for the wrapper module
    em = _load("refds.evaluator_models", os.path.join(ref, "datasets1", "evaluator_models.py"))
    metrics = _load("ref_metrics", os.path.join(ref, "utils", "metrics.py"))
    pkg = types.ModuleType("refds")
    pkg.__path__ = [os.path.join(ref, "datasets1")]
    sys.modules["refds"] = pkg
    sys.modules.setdefault("models", types.SimpleNamespace(MotionTransformer=None))
    wrapper = _load("refds.evaluator", os.path.join(ref, "datasets1", "evaluator.py"), package="refds").EvaluatorModelWrapper
    return em, metrics, wrapper


def run_wrapper(em, wrapper, case):
    d = dict(ER.DEFAULT_DIMS, **case["dims"])
    state = ER.synth_state(case["dims"], case["seed"])
    mov = em.MovementConvEncoder(d["dim_pose"] - 4, d["dim_movement_enc_hidden"], d["dim_movement_latent"])
    txt = em.TextEncoderBiGRUCo(d["dim_word"], d["dim_pos_ohot"], d["dim_text_hidden"], d["dim_coemb_hidden"], "cpu")
    mot = em.MotionEncoderBiGRUCo(d["dim_movement_latent"], d["dim_motion_hidden"], d["dim_coemb_hidden"], "cpu")
    for m, k in ((mov, "movement_encoder"), (txt, "text_encoder"), (mot, "motion_encoder")):
        m.load_state_dict(state[k], strict=True)
        m.eval()
    w, p, x = ER.synth_inputs(case["B"], case["T"], case["dims"], case["seed"])
    ns = types.SimpleNamespace(device="cpu", opt=types.SimpleNamespace(unit_length=4), movement_encoder=mov,
                               text_encoder=txt, motion_encoder=mot)
    m_lens, cap_lens = torch.tensor(case["m_lens"]), torch.tensor(case["cap_lens"])
    t_emb, m_emb = wrapper.get_co_embeddings(ns, w, p, cap_lens, x, m_lens)
    with torch.no_grad():
        mv = mov(x[ER.align_index(m_lens)][..., :-4])
    # the restatement agrees (the tests pin it to these numbers at 1e-6)
    rt, rm, rmv = ER.co_embeddings(state, w, p, cap_lens, x, m_lens)
    for a, b in ((t_emb, rt), (m_emb, rm), (mv, rmv)):
        e = float((a.double() - b).abs().max() / b.abs().max())
        assert e < 1e-5, e
    return t_emb.numpy(), m_emb.numpy(), mv.numpy()


def run_metrics(metrics):
    c = METRICS
    s = c["seed"]
    t = ER.synth_embeddings((c["n_pairs"], 512), "text", s).numpy()
    m = (ER.synth_embeddings((c["n_pairs"], 512), "motion", s, 0.6) + torch.from_numpy(t) * 0.5).numpy()
    score, counts, size = 0.0, np.zeros(3, np.int64), 0
    for i in range(0, c["n_pairs"] // c["batch_size"] * c["batch_size"], c["batch_size"]):
        dm = metrics.euclidean_distance_matrix(t[i:i + c["batch_size"]], m[i:i + c["batch_size"]])
        # no near-ties around any true pair: the GPU ranks must be exact
        gap = np.abs(dm - np.diag(dm)[:, None]) + np.eye(len(dm)) * 1e9
        assert gap.min() > 1e-3 * np.abs(dm).max(), gap.min()
        score += dm.trace()
        counts += metrics.calculate_top_k(np.argsort(dm, axis=1), top_k=3).sum(axis=0)
        size += len(dm)
    gt = ER.synth_embeddings((c["n_gt"], 512), "gt", s).numpy()
    gen = ER.synth_embeddings((c["n_gen"], 512), "gen", s, 0.8, 0.05).numpy()
    mu1, s1 = metrics.calculate_activation_statistics(gt)
    mu2, s2 = metrics.calculate_activation_statistics(gen)
    fid = metrics.calculate_frechet_distance(mu1, s1, mu2, s2)
    div_x = ER.synth_embeddings((c["n_div"], 512), "div", s).numpy()
    np.random.seed(c["div_seed"])
    div = metrics.calculate_diversity(div_x, c["div_times"])
    mm_x = ER.synth_embeddings(c["mm"] + (512,), "mm", s).numpy()
    np.random.seed(c["mm_seed"])
    mm = metrics.calculate_multimodality(mm_x, c["mm_times"])
    return dict(matching_score=np.float64(score / size), r_counts=counts.astype(np.int64), r_size=np.int64(size),
                fid=np.float64(fid), diversity=np.float64(div), multimodality=np.float64(mm))


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/make_evaluator_golden.py REFERENCE_DIR  (the reference's text2motion/ directory)")
    ref = sys.argv[1]
    em, metrics, wrapper = reference(ref)
    torch.set_grad_enabled(False)
    out = {}
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):  # the reference's calculate_top_k prints
        for tag, case in (("a", CASE_A), ("a2", CASE_A2), ("b", CASE_B)):
            t, m, mv = run_wrapper(em, wrapper, case)
            out[f"{tag}_text"], out[f"{tag}_motion"] = t, m
            if tag != "b":
                out[f"{tag}_movements"] = mv
        for k, v in run_metrics(metrics).items():
            out[f"c_{k}"] = v
    d = ER.DEFAULT_DIMS
    mods = {"movement_encoder": em.MovementConvEncoder(d["dim_pose"] - 4, 512, 512),
            "text_encoder": em.TextEncoderBiGRUCo(300, 15, 512, 512, "cpu"),
            "motion_encoder": em.MotionEncoderBiGRUCo(512, 1024, 512, "cpu")}
    layout = {k: [[n, list(v.shape)] for n, v in m.state_dict().items()] for k, m in mods.items()}
    meta = {"cases": {"a": CASE_A, "a2": CASE_A2, "b": CASE_B}, "metrics": METRICS, "layout": layout}
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "evaluator.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
