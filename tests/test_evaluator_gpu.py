"""GPU: the text-motion evaluator (csrc/evaluator.hip + mdm_gemm) against the reference's outputs (tests/golden/evaluator.npz)
and the fp64 restatement (tests/evaluator_ref.py); the metrics; the generation-for-evaluation driver end to end."""
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, build_module, load_golden, pkg, rel_inf
import evaluator_ref as ER

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "evaluator.npz"))
    return g, json.loads(str(g["meta"]))


def _evaluator(dims, seed):
    E = pkg("evaluator")
    ev = E.MotionTextEvaluator(**dims)
    st = ER.synth_state(dims, seed)
    for k in ("movement_encoder", "text_encoder", "motion_encoder"):
        getattr(ev, k).load_state_dict(st[k], strict=True)
    return ev.cuda().eval(), st


def _t(a):
    return a.detach().cpu().double() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a)).double()


def _rel(a, b):
    return rel_inf(_t(a), _t(b))


@pytest.mark.parametrize("tag", ["a", "a2", "b"])
def test_embeddings_match_reference_golden(golden, tag):
    g, meta = golden
    case = meta["cases"][tag]
    ev, _ = _evaluator(case["dims"], case["seed"])
    w, p, x = ER.synth_inputs(case["B"], case["T"], case["dims"], case["seed"])
    m_lens, cap_lens = torch.tensor(case["m_lens"]), torch.tensor(case["cap_lens"])
    t, m = ev.get_co_embeddings(w.cuda(), p.cuda(), cap_lens, x.cuda(), m_lens)
    assert _rel(t, g[f"{tag}_text"]) <= TOL
    assert _rel(m, g[f"{tag}_motion"]) <= TOL
    assert _rel(ev.get_motion_embeddings(x.cuda(), m_lens), g[f"{tag}_motion"]) <= TOL
    if f"{tag}_movements" in g:
        idx = torch.from_numpy(ER.align_index(m_lens))
        mv = ev.movement_encoder.encode(x.cuda(), feats=x.shape[-1] - 4).cpu()[idx]
        assert _rel(mv, g[f"{tag}_movements"]) <= TOL


@pytest.fixture(scope="module")
def full_evaluators():
    return {263: _evaluator({}, 41), 251: _evaluator(dict(dim_pose=251), 42)}


@pytest.mark.parametrize("name,dim_pose,m_lens,cap_lens", [
    ("ragged_unsorted", 263, [52, 196, 4, 131, 88], [7, 22, 1, 15, 10]),
    ("equal", 263, [120, 120, 120], [9, 9, 9]),
    ("ties", 263, [64, 196, 64, 8, 196], [3, 12, 22, 5, 12]),
    ("kit", 251, [196, 40, 97, 4], [22, 4, 11, 2]),
    ("len_1_and_T", 263, [4, 196], [1, 22]),
])
def test_reference_widths_against_restatement(full_evaluators, name, dim_pose, m_lens, cap_lens):
    ev, st = full_evaluators[dim_pose]
    B, T = len(m_lens), 196
    w, p, x = ER.synth_inputs(B, T, dict(dim_pose=dim_pose), 50 + len(name))
    ml, cl = torch.tensor(m_lens), torch.tensor(cap_lens)
    t, m = ev.get_co_embeddings(w.cuda(), p.cuda(), cl, x.cuda(), ml)
    rt, rm, _ = ER.co_embeddings(st, w, p, cl, x, ml)
    assert _rel(t, rt) <= TOL, name
    assert _rel(m, rm) <= TOL, name
    # the output order is the reference's align_idx rule, ties included
    want = np.argsort(ml.data.tolist())[::-1].copy()
    assert (ev.align_index(ml) == want).all()
    tt = ev.text_encoder.encode(w.cuda(), p.cuda(), cl).cpu()
    assert _rel(t, tt[torch.from_numpy(want)]) <= 1e-6


def _metric_sets(c):
    s = c["seed"]
    t = ER.synth_embeddings((c["n_pairs"], 512), "text", s)
    m = ER.synth_embeddings((c["n_pairs"], 512), "motion", s, 0.6) + t * 0.5
    gt = ER.synth_embeddings((c["n_gt"], 512), "gt", s)
    gen = ER.synth_embeddings((c["n_gen"], 512), "gen", s, 0.8, 0.05)
    div = ER.synth_embeddings((c["n_div"], 512), "div", s)
    mm = ER.synth_embeddings(tuple(c["mm"]) + (512,), "mm", s)
    return t, m, gt, gen, div, mm


def test_metrics_match_reference_golden(golden):
    g, meta = golden
    c = meta["metrics"]
    M = pkg("eval_metrics")
    t, m, gt, gen, div, mm = (v.cuda() for v in _metric_sets(c))
    r = M.matching_and_r_precision(t, m, c["batch_size"])
    assert r["size"] == int(g["c_r_size"])
    assert (r["r_precision_counts"] == g["c_r_counts"]).all(), (r["r_precision_counts"], g["c_r_counts"])
    assert abs(r["matching_score"] / float(g["c_matching_score"]) - 1) <= 1e-5
    mu1, s1 = M.activation_stats(gt)
    mu2, s2 = M.activation_stats(gen)
    fid = M.frechet_distance(mu1, s1, mu2, s2)
    assert abs(fid / float(g["c_fid"]) - 1) <= 1e-4, (fid, float(g["c_fid"]))
    d = M.diversity(div, c["div_times"], seed=c["div_seed"])
    assert abs(d / float(g["c_diversity"]) - 1) <= 1e-5
    # np.random.seed + np.random.choice (the reference) draws what RandomState(seed).choice draws
    np.random.seed(c["div_seed"])
    assert M.diversity(div, c["div_times"]) == d
    mmv = M.multimodality(mm, c["mm_times"], seed=c["mm_seed"])
    assert abs(mmv / float(g["c_multimodality"]) - 1) <= 1e-5


def test_matching_kernel_distances_and_ranks():
    M = pkg("eval_metrics")
    t = ER.synth_embeddings((40, 512), "mk_t", 1).cuda()
    m = ER.synth_embeddings((40, 512), "mk_m", 1).cuda()
    rank, diag, dist = M._match(t, m, with_dist=True)
    want = ER.dist_matrix(t.cpu().numpy(), m.cpu().numpy())
    assert _rel(dist, want) <= 1e-6
    assert _rel(diag, np.diag(want)) <= 1e-6
    assert (rank.cpu().numpy() == (want < np.diag(want)[:, None]).sum(1)).all()


def test_from_checkpoint_reference_layout(tmp_path):
    E = pkg("evaluator")
    dims = dict(dim_text_hidden=32, dim_motion_hidden=48, dim_movement_enc_hidden=64, dim_movement_latent=64,
                dim_coemb_hidden=64)
    st = ER.synth_state(dims, 7)
    path = tmp_path / "finest.tar"
    torch.save({**st, "epoch": 123}, path)
    ev = E.MotionTextEvaluator.from_checkpoint(str(path), device="cuda", **dims)
    assert ev.epoch == 123
    w, p, x = ER.synth_inputs(3, 24, dims, 7)
    ml, cl = torch.tensor([24, 9, 16]), torch.tensor([10, 22, 4])
    t, m = ev.get_co_embeddings(w, p, cl, x, ml)
    rt, rm, _ = ER.co_embeddings(st, w, p, cl, x, ml)
    assert _rel(t, rt) <= TOL and _rel(m, rm) <= TOL
    # a changed parameter invalidates the packs
    with torch.no_grad():
        ev.motion_encoder.output_net[3].bias.add_(1.0)
    m2 = ev.get_motion_embeddings(x, ml)
    assert _rel(m2.cpu() - 1.0, rm) <= TOL
    bad = {k: v for k, v in st["text_encoder"].items() if k != "hidden"}
    torch.save({**st, "text_encoder": bad, "epoch": 1}, path)
    with pytest.raises(RuntimeError):
        E.MotionTextEvaluator.from_checkpoint(str(path), device="cuda", **dims)


def test_generate_for_evaluation_end_to_end():
    g, meta = load_golden("loops_tiny")
    m, _ = build_module(meta, precision=3)
    m.set_uncond_embedding(g["xf_proj_uncond"][:1].cuda(), g["xf_out_uncond"][:1].cuda())
    m.text_encoder_fn = lambda text, device: (g["xf_proj"][:1].expand(len(text), -1).to(device),
                                              g["xf_out"][:1].expand(len(text), -1, -1).to(device))
    Tr, M = pkg("trainer"), pkg("eval_metrics")
    args = types.SimpleNamespace(device=torch.device("cuda"), diffusion_steps=25, is_train=False, cfg_scale=2.5)
    tr = Tr.DDPMTrainer(args, m)
    N, T = 8, 16
    caps = [f"caption {i}" for i in range(N)]
    raw = torch.tensor([16, 9, 13, 5, 16, 12, 11, 14])
    out = tr.generate_for_evaluation(caps, raw, 263, mm_num_samples=2, mm_num_repeats=3, unit_length=1, max_motion_length=T,
                                     seed=5, batch_size=4, sampler="dpmpp2m", sample_steps=5)
    lens = out["m_lens"]
    assert lens.tolist() == [16, 10, 13, 10, 16, 12, 11, 14]  # max(m, 10 unit), capped at max_motion_length
    mm_idxs = np.sort(np.random.RandomState(5).choice(N, 2, replace=False))
    assert (out["mm_idxs"] == mm_idxs).all()
    assert out["motions"].shape == (N, T, 263) and out["mm_motions"].shape == (2, 3, T, 263)
    # frames at or past each length are zero; valid frames equal generate_bucketed(seed=) on the same caption list
    all_cap, all_len = [], []
    for i in range(N):
        for _ in range(3 if i in set(mm_idxs.tolist()) else 1):
            all_cap.append(caps[i])
            all_len.append(int(lens[i]))
    ref = tr.generate_bucketed(all_cap, torch.tensor(all_len), 263, 4, unit_length=1, seed=5, sampler="dpmpp2m", sample_steps=5)
    first = np.cumsum([0] + [3 if i in set(mm_idxs.tolist()) else 1 for i in range(N)])[:-1]
    for i in range(N):
        n = int(lens[i])
        assert torch.equal(out["motions"][i, :n], ref[first[i]][:n])
        assert not out["motions"][i, n:].any()
    for k, i in enumerate(mm_idxs.tolist()):
        for r in range(3):
            assert torch.equal(out["mm_motions"][k, r, :lens[i]], ref[first[i] + r][:lens[i]])
    # the five metrics on a small evaluator
    dims = dict(dim_text_hidden=32, dim_motion_hidden=48, dim_movement_enc_hidden=64, dim_movement_latent=64,
                dim_coemb_hidden=64)
    ev, _ = _evaluator(dims, 9)
    w, p, _ = ER.synth_inputs(N, T, dims, 9)
    gt_x = ER.synth_inputs(N, T, dims, 10)[2]
    res = M.evaluate_motions(ev, {"motions": gt_x, "m_lens": lens},
                             {"word_embs": w, "pos_ohot": p, "cap_lens": torch.full((N,), 12), "motions": out["motions"],
                              "m_lens": lens},
                             {"motions": out["mm_motions"], "m_lens": out["mm_lens"]},
                             batch_size=4, diversity_times=4, mm_times=2, seed=0)
    assert set(res) == {"Matching Score", "R_precision", "FID", "Diversity", "MultiModality"}
    vals = [res["Matching Score"], res["FID"], res["Diversity"], res["MultiModality"]] + res["R_precision"]
    assert all(np.isfinite(v) for v in vals), res
    assert res["R_precision"][0] <= res["R_precision"][1] <= res["R_precision"][2] <= 1.0
