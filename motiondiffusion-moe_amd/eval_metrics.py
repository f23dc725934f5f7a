"""The five text-to-motion metrics (tools/evaluation.py:144-326, utils/metrics.py) on the HIP library: Matching Score and
R-precision top-1..3 (mdm_eval_matching), FID (mean / covariance on the device: mdm_eval_center + an F32_KSTRIDE mdm_gemm;
the 512 x 512 matrix square root's trace on the host in fp64), Diversity and MultiModality (the pair distances are the
diagonal of mdm_eval_matching on the drawn rows)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from .ops import f32_operand, gemm_desc, run_gemm


def _dev(x, device=None) -> torch.Tensor:
    t = torch.as_tensor(x)
    if device is None:
        device = t.device if t.is_cuda else "cuda"
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _match(text: torch.Tensor, motion: torch.Tensor, with_dist: bool = False):
    """(rank (B,) int32, diag (B,) fp32[, dist (B, B)]) of one batch of pairs, one launch."""
    B, D = text.shape
    rank = torch.empty(B, dtype=torch.int32, device=text.device)
    diag = torch.empty(B, dtype=torch.float32, device=text.device)
    dist = torch.empty(B, B, dtype=torch.float32, device=text.device) if with_dist else None
    L.check(L.lib().mdm_eval_matching(text.data_ptr(), motion.data_ptr(), B, D, L.ptr(dist), rank.data_ptr(), diag.data_ptr(),
                                      L.stream_ptr()), "mdm_eval_matching")
    return (rank, diag, dist) if with_dist else (rank, diag)


def pair_distances(a, b) -> torch.Tensor:
    """||a_i - b_i||_2 for matching rows of a, b (N, D) on the device."""
    a, b = _dev(a), _dev(b)
    a, b = a, b.to(a.device)
    return _match(a, b)[1]


def matching_and_r_precision(text_emb, motion_emb, batch_size: int = 32, top_k: int = 3) -> Dict:
    """tools/evaluation.py:144-200: the embeddings split into consecutive batches of ``batch_size`` pairs (the last partial
    batch dropped, like the reference's loader); per batch the true pair's rank among the batch's motions.
    Returns matching score (mean diagonal distance), R-precision top-1..top_k and the integer counts behind it."""
    t = _dev(text_emb)
    m = _dev(motion_emb, t.device)
    nb = t.shape[0] // batch_size
    if nb == 0:
        raise ValueError(f"need at least one full batch of {batch_size} pairs")
    ranks, diags = [], []
    for i in range(nb):
        r, d = _match(t[i * batch_size:(i + 1) * batch_size], m[i * batch_size:(i + 1) * batch_size])
        ranks.append(r)
        diags.append(d)
    rank = torch.cat(ranks).cpu().numpy()
    diag = torch.cat(diags).cpu().numpy().astype(np.float64)
    n = nb * batch_size
    counts = np.array([(rank < k).sum() for k in range(1, top_k + 1)], dtype=np.int64)
    return {"matching_score": float(diag.sum() / n), "r_precision": counts / n, "r_precision_counts": counts, "size": n}


def activation_stats(emb):
    """(mean (D,), covariance (D, D) with 1 / (N - 1)), computed on the device, returned as fp64 host arrays
    (utils/metrics.py:60-70)."""
    x = _dev(emb)
    N, D = x.shape
    if N < 2:
        raise ValueError("the covariance needs at least two samples")
    mean = torch.empty(D, dtype=torch.float32, device=x.device)
    xc = torch.empty_like(x)
    lib = L.lib()
    L.check(lib.mdm_eval_center(x.data_ptr(), N, D, mean.data_ptr(), xc.data_ptr(), L.stream_ptr()), "mdm_eval_center")
    cov = torch.empty(D, D, dtype=torch.float32, device=x.device)
    d = gemm_desc(L.PREC_X3)  # cov[m, n] = sum_k xc[k, m] xc[k, n] / (N - 1): both operands read k-strided
    d.A = f32_operand(xc, D, L.OP_F32_KSTRIDE)
    d.W = f32_operand(xc, D, L.OP_F32_KSTRIDE)
    d.M, d.N, d.K = D, D, N
    d.C, d.ldc = cov.data_ptr(), D
    d.alpha = 1.0 / (N - 1)
    run_gemm(d)
    return mean.cpu().double().numpy(), cov.cpu().double().numpy()


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """||mu1 - mu2||^2 + tr(S1) + tr(S2) - 2 tr sqrtm(S1 S2) in fp64 on the host (utils/metrics.py:95-150).
    tr sqrtm(S1 S2) = sum_i sqrt(lambda_i(S1^1/2 S2 S1^1/2)), eigenvalues clamped at 0: scipy.linalg.sqrtm's value for
    positive semi-definite S1, S2, without scipy."""
    mu1, mu2 = (torch.as_tensor(np.asarray(v), dtype=torch.float64) for v in (mu1, mu2))
    s1, s2 = (torch.as_tensor(np.asarray(v), dtype=torch.float64) for v in (sigma1, sigma2))
    assert mu1.shape == mu2.shape and s1.shape == s2.shape
    s1 = 0.5 * (s1 + s1.T)
    s2 = 0.5 * (s2 + s2.T)
    lam, V = torch.linalg.eigh(s1)
    r1 = (V * lam.clamp(min=0).sqrt()) @ V.T
    mid = r1 @ s2 @ r1
    ev = torch.linalg.eigvalsh(0.5 * (mid + mid.T)).clamp(min=0)
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(s1) + torch.trace(s2) - 2 * ev.sqrt().sum())


def _draw(n: int, times: int, seed, indices):
    if indices is not None:
        first, second = (np.asarray(i) for i in indices)
        return first, second
    rs = np.random.RandomState(seed) if seed is not None else np.random.mtrand._rand
    return rs.choice(n, times, replace=False), rs.choice(n, times, replace=False)


def diversity(emb, times: int, seed: Optional[int] = None, indices=None) -> float:
    """utils/metrics.py:73-81: mean distance between ``times`` random pairs of rows.  The two index draws are
    ``RandomState(seed).choice(N, times, replace=False)`` (without seed: numpy's global state, as the reference);
    ``indices`` = (first, second) overrides them."""
    x = _dev(emb)
    N = x.shape[0]
    if N <= times:
        raise ValueError(f"diversity needs more than {times} samples (got {N})")
    first, second = _draw(N, times, seed, indices)
    i1 = torch.as_tensor(first, dtype=torch.long, device=x.device)
    i2 = torch.as_tensor(second, dtype=torch.long, device=x.device)
    d = pair_distances(x.index_select(0, i1), x.index_select(0, i2))
    return float(d.cpu().double().mean())


def multimodality(emb, times: int, seed: Optional[int] = None, indices=None) -> float:
    """utils/metrics.py:84-92: emb (n_prompts, R, D); mean distance between ``times`` random pairs of the R motions of
    each prompt (the same index pairs for every prompt)."""
    x = _dev(emb)
    P, R, D = x.shape
    if R <= times:
        raise ValueError(f"multimodality needs more than {times} motions per prompt (got {R})")
    first, second = _draw(R, times, seed, indices)
    i1 = torch.as_tensor(first, dtype=torch.long, device=x.device)
    i2 = torch.as_tensor(second, dtype=torch.long, device=x.device)
    a = x.index_select(1, i1).reshape(-1, D).contiguous()
    b = x.index_select(1, i2).reshape(-1, D).contiguous()
    return float(pair_distances(a, b).cpu().double().mean())


def metric_statistics(values):
    """tools/evaluation.py:322-326: (mean, 1.96 std / sqrt(n)) over n replications (axis 0)."""
    v = np.asarray(values, dtype=np.float64)
    return v.mean(axis=0), 1.96 * v.std(axis=0) / np.sqrt(v.shape[0])


def _batches(n: int, batch_size: int, drop_last: bool):
    stop = n // batch_size * batch_size if drop_last else n
    return [(i, min(i + batch_size, n)) for i in range(0, stop, batch_size)]


@torch.no_grad()
def evaluate_motions(evaluator, gt: Dict, generated: Dict, mm: Optional[Dict] = None, *, batch_size: int = 32,
                     diversity_times: int = 300, mm_times: int = 10, seed: Optional[int] = None) -> Dict:
    """The five metrics of one evaluation replication (tools/evaluation.py:144-320) on tensor sets:
      gt        {"motions": (N, T, dim_pose), "m_lens": (N,)}                       ground-truth motions (FID reference)
      generated {"word_embs", "pos_ohot", "cap_lens", "motions", "m_lens"}         generated motions with their captions
      mm        {"motions": (P, R, T, dim_pose), "m_lens": (P, R)} or None         R generations of each of P captions
    Both sets go through the evaluator in consecutive batches of ``batch_size`` (the last partial batch dropped, as the
    reference's loaders).  ``seed`` seeds the diversity / multimodality index draws (None: numpy's global state)."""
    gen_t, gen_m, gt_m = [], [], []
    for a, b in _batches(generated["motions"].shape[0], batch_size, True):
        t, m = evaluator.get_co_embeddings(generated["word_embs"][a:b], generated["pos_ohot"][a:b],
                                           torch.as_tensor(generated["cap_lens"])[a:b], generated["motions"][a:b],
                                           torch.as_tensor(generated["m_lens"])[a:b])
        gen_t.append(t)
        gen_m.append(m)
    for a, b in _batches(gt["motions"].shape[0], batch_size, True):
        gt_m.append(evaluator.get_motion_embeddings(gt["motions"][a:b], torch.as_tensor(gt["m_lens"])[a:b]))
    text_emb, motion_emb, gt_emb = torch.cat(gen_t), torch.cat(gen_m), torch.cat(gt_m)
    ms = matching_and_r_precision(text_emb, motion_emb, batch_size)
    mu_g, cov_g = activation_stats(gt_emb)
    mu, cov = activation_stats(motion_emb)
    out = {"Matching Score": ms["matching_score"], "R_precision": [float(v) for v in ms["r_precision"]],
           "FID": frechet_distance(mu_g, cov_g, mu, cov),
           "Diversity": diversity(motion_emb, diversity_times, seed=seed)}
    if mm is not None:
        P = mm["motions"].shape[0]
        emb = torch.stack([evaluator.get_motion_embeddings(mm["motions"][p], torch.as_tensor(mm["m_lens"])[p]) for p in range(P)])
        out["MultiModality"] = multimodality(emb, mm_times, seed=None if seed is None else seed + 1)
    else:
        out["MultiModality"] = 0.0  # the reference's value without multimodality samples (evaluation.py:306-307)
    return out
