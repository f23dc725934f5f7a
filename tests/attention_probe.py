"""Probe fixtures for the attention tests: inputs on which an attention core that masks, pairs or maps features wrongly moves
the result, deliberately wrong variants ("mutants") of the oracle's attention functions, metrics that the residual does not swamp,
and the oracle with a rounding hook from which the branch tolerances of the GPU tests are measured.

CPU only.  Everything is the oracle (oracle/denoiser_ref.py) with one of its module-level functions swapped for the time of a
call; `fast_attention_variant` restates `fast_attention` line by line with switches (tests/test_attention_probe_host.py asserts
that it equals the oracle's bit for bit with the switches off).  Nothing here is imported by the package.

tests/test_attention_probe_host.py proves the power of every GPU case of tests/test_attention_selective_gpu.py from this module
alone: every mutant that belongs to a block is at least POWER x the tolerance away from the true oracle."""
import contextlib
import os
import sys

import torch
import torch.nn.functional as F

from conftest import ROOT, golden_state, load_golden, pkg

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import denoiser_ref as R  # noqa: E402

PRE = "decoder_blocks_low.0.module"
POWER = 4.0  # a mutant must be at least this many tolerances away from the oracle (a condition, not a measurement)


@contextlib.contextmanager
def oracle_with(**fns):
    """Swap module-level functions of the oracle (looked up at call time by its own callers) for the time of a block."""
    old = {k: getattr(R, k) for k in fns}
    try:
        for k, f in fns.items():
            setattr(R, k, f)
        yield
    finally:
        for k, f in old.items():
            setattr(R, k, f)


# ------------------------------------------------------------------------------------------------------------------------
# the Performer core with switches
# ------------------------------------------------------------------------------------------------------------------------
_FA = R.fast_attention
_STATE = R.linear_cross_text_state
_LIN = R._lin


def fast_attention_variant(q, k, v, mask, nw, nb, P, eps=1e-6, *, clamp=True, textbook_den=False, kperm=None, rnd=None, record=None):
    """oracle fast_attention, statement by statement, with: the +-15 clamp optional, the textbook denominator q~ . sum_t k~[t]
    instead of the same-frame dot, K's features on a column permutation of P, `rnd` applied wherever the 16-bit cores hold a
    16-bit image (csrc/perf_attn.hip header: the normalised q / k fragments, P^T, kphi^T, v, the KV^T state, the packed q
    features of the numerator, the attention rows), `record(zq, zk)` seeing the feature logits."""
    r = rnd if rnd is not None else (lambda t: t)
    dh = q.shape[-1]
    ln = lambda z: F.layer_norm(z, (dh,), nw, nb, 1e-5)
    q, k, v = ln(q), ln(k), ln(v)
    q = r(F.normalize(q, dim=-1))
    k = r(F.normalize(k, dim=-1))
    v = r(v)
    Pq = r(P)
    Pk = Pq if kperm is None else Pq[:, kperm]
    zq, zk = q @ Pq, k @ Pk
    if record is not None:
        record(zq, zk)
    if clamp:
        zq, zk = torch.clamp(zq, -15, 15), torch.clamp(zk, -15, 15)
    qf = torch.exp(zq) * 0.1
    kf = torch.exp(zk) * 0.1
    kf = r(kf * mask[:, None, :, None].to(kf.dtype))
    kv = r((kf.transpose(-1, -2) @ v) * 0.1)
    num = (r(qf) @ kv) * 0.1
    if textbook_den:
        den = (qf * kf.sum(-2, keepdim=True)).sum(-1, keepdim=True).clamp(min=eps)
    else:
        den = (qf * kf).sum(-1, keepdim=True).clamp(min=eps)
    return r(ln(num / den))


def _relen(fn):
    """fast_attention with every sample's length replaced by fn(length), kept inside [0, S]."""
    def fa(q, k, v, mask, nw, nb, P, eps=1e-6):
        S = mask.shape[1]
        n = fn(mask.sum(1).long()).clamp(0, S)
        return _FA(q, k, v, R.src_mask(S, n), nw, nb, P, eps)
    return fa


def _feature_perm(m):
    return torch.arange(m).roll(1)


PERFORMER_MUTANTS = {
    "mask ignored": lambda q, k, v, mask, *a: _FA(q, k, v, torch.ones_like(mask), *a),
    "length rounded up to 16": _relen(lambda n: (n + 15) // 16 * 16),
    "length rounded up to 32": _relen(lambda n: (n + 31) // 32 * 32),
    "length + 1": _relen(lambda n: n + 1),
    "length - 1": _relen(lambda n: n - 1),
    "K heads rolled against V": lambda q, k, v, *a: _FA(q, k.roll(1, 1), v, *a),
    "K frames rolled against V": lambda q, k, v, *a: _FA(q, k.roll(1, 2), v, *a),
    "K features on permuted columns of P": lambda q, k, v, mask, nw, nb, P, eps=1e-6: fast_attention_variant(
        q, k, v, mask, nw, nb, P, eps, kperm=_feature_perm(P.shape[1])),
    "clamp removed": lambda *a: fast_attention_variant(*a, clamp=False),
    "textbook denominator": lambda *a: fast_attention_variant(*a, textbook_den=True),
}
# the clamp only acts where a logit passes +-15: that mutant belongs to the `clamp` fixture alone
CLAMP_ONLY = ("clamp removed",)


def _state_wrong_axis(xf, sd, prefix, H):
    B, N, _ = xf.shape
    tn = R._ln(xf, sd, prefix + ".text_norm")
    k = F.softmax(R._lin(tn, sd, prefix + ".key").view(B, N, H, -1), dim=-1)
    v = R._lin(tn, sd, prefix + ".value").view(B, N, H, -1)
    return torch.einsum("bnhd,bnhl->bhdl", k, v)


# linear cross-attention: (text-state function or None, token-count function or None; None = the true one)
XATTN_MUTANTS = {
    "text softmax over the wrong axis": (_state_wrong_axis, None),
    "text state of head h used for head h+1": (lambda *a: _STATE(*a).roll(1, 1), None),
    "text state transposed": (lambda *a: _STATE(*a).transpose(-1, -2), None),
    "token count ignored": (None, lambda n, N: N),
    "token count + 1": (None, lambda n, N: min(n + 1, N)),
}


def _roll_key_heads(sd, prefix, H):
    out = dict(sd)
    for s in (".key.weight", ".key.bias"):
        w = sd[prefix + s]
        out[prefix + s] = w.roll(w.shape[0] // H, 0)
    return out


def _drop_scale(sd, prefix, H):
    out = dict(sd)
    dh = sd[prefix + ".query.weight"].shape[0] // H
    for s in (".query.weight", ".query.bias"):
        out[prefix + s] = sd[prefix + s] * dh ** 0.5
    return out


# softmax cross-attention: (state-dict rewrite or None, token-count function or None)
SD_MUTANTS = {
    "token count ignored": (None, lambda n, N: N),
    "token count + 1": (None, lambda n, N: min(n + 1, N)),
    "K heads rolled against V": (_roll_key_heads, None),
    "scale dropped": (_drop_scale, None),
}


# ------------------------------------------------------------------------------------------------------------------------
# fixtures
# ------------------------------------------------------------------------------------------------------------------------
# Feature-logit gain on P per fixture variant.  `mid`: |z P| <= 8 everywhere (asserted), valid in all four modes.  `clamp`: a
# measured share of the logits lies beyond +-15 (asserted), where 0.1 e^15 = 3.3e5 does not fit fp16: modes 3, 4 and 1 only.
P_GAIN = {"mid": 64.0, "clamp": 200.0}
STYLE_GAIN = 30.0  # on out_layers.2 of both Performers' stylizations: the branch is 0.1 * this of the residual, not 1 %
XQ_GAIN, XK_GAIN, SDQ_GAIN = 4.0, 4.0, 4.0  # query / key of the linear cross-attention, query of the softmax one
_WIDTHS = {"small": "fwd_small_dims", "big": "fwd_big_dims"}
_FIX = {}


def selective_state(width="small", variant="mid"):
    """(sd, eph, proj, H, D, Dt) of the golden case with layer 0 of both scales rewritten so that the attention is selective:
    key = query in both Performers (q . k of two frames = cosine of their normalised queries), P scaled by P_GAIN[variant],
    the cross-attention logits spread by XQ / XK / SDQ_GAIN.  Memoised; treat the tensors as read-only."""
    if (width, variant) not in _FIX:
        _, meta = load_golden(_WIDTHS[width])
        sd, eph, proj, mcfg = golden_state(meta)
        for scale in ("low", "high"):
            pre = f"decoder_blocks_{scale}.0.module"
            for slot in ("local", "global"):
                p = f"{pre}.dual_self_attn.{slot}_attn"
                sd[p + ".key.weight"], sd[p + ".key.bias"] = sd[p + ".query.weight"], sd[p + ".query.bias"]
                proj[f"{scale}.0.{slot}"] = proj[f"{scale}.0.{slot}"] * P_GAIN[variant]
                for t in (".style_block.out_layers.2.weight", ".style_block.out_layers.2.bias"):
                    sd[p + t] = sd[p + t] * STYLE_GAIN
            for key, gain in ((".cross_attn.base_ca.query", XQ_GAIN), (".cross_attn.base_ca.key", XK_GAIN),
                              (".sd_cross_attn.query", SDQ_GAIN)):
                for s in (".weight", ".bias"):
                    sd[pre + key + s] = sd[pre + key + s] * gain
        Dt = sd[PRE + ".sd_cross_attn.key.weight"].shape[1]
        _FIX[width, variant] = (sd, eph, proj, mcfg["num_heads"], mcfg["latent_dim"], Dt, meta)
    return _FIX[width, variant]


NCLUSTER = 6


def _clustered_rows(B, S, D, count, name, pad_gain):
    """(B, S, D) rows and their cluster ids: frame t of sample b belongs to cluster (t + 2 b) % 6, the clusters are +-3
    seeded directions (so the normalised queries of two clusters meet at about +1, 0 or -1) plus 15 % noise; rows at or past
    count[b] hold a seventh direction at `pad_gain` times the amplitude, with their cluster's direction mixed in (so the
    queries of that cluster attend to them) -- content unlike every valid row."""
    synth = pkg("synth")
    dirs = synth.uniform_pm1((4, D), name + ".dirs", D) * (3.0 ** 0.5)
    centres = torch.stack([dirs[0], -dirs[0], dirs[1], -dirs[1], dirs[2], -dirs[2]])
    cid = (torch.arange(S)[None, :] + 2 * torch.arange(B)[:, None]) % NCLUSTER
    rows = centres[cid] + 0.15 * (3.0 ** 0.5) * synth.uniform_pm1((B, S, D), name + ".noise", S)
    pad = pad_gain * (dirs[3] + centres[cid.roll(1, 1)] + 0.15 * (3.0 ** 0.5) * synth.uniform_pm1((B, S, D), name + ".padnoise", S))
    past = torch.arange(S)[None, :] >= torch.as_tensor(count)[:, None]
    return torch.where(past[..., None], pad, rows), cid


def style_rows(sd, eph, emb):
    """(4, B, 2D): the (scale | shift) rows of the four stylizations of layer low.0, as mdm_block_forward takes them."""
    sc = []
    for slot, sp in (("local_style", PRE + ".dual_self_attn.local_attn.style_block"),
                     ("global_style", PRE + ".dual_self_attn.global_attn.style_block"),
                     ("cross_style", PRE + ".cross_attn.base_ca.proj_out"), ("ffn_style", PRE + ".ffn.proj_out")):
        w, b = eph["low.0." + slot]
        sc.append(F.linear(F.silu(F.linear(emb, w, b)), sd[sp + ".emb_layers.1.weight"], sd[sp + ".emb_layers.1.bias"]))
    return torch.stack(sc)


_INP = {}


def selective_inputs(width, S, lengths, N=6, ntok=None):
    """Inputs of one case (memoised): clustered motion rows with unlike rows past each length, clustered text rows with unlike
    rows past each token count.  Independent of the fixture variant."""
    key = (width, S, tuple(lengths), N, None if ntok is None else tuple(ntok))
    if key not in _INP:
        sd, eph, proj, H, D, Dt, _ = selective_state(width)
        B = len(lengths)
        synth = pkg("synth")
        h, cid = _clustered_rows(B, S, D, lengths, "probe.h", 4.0)
        nt = list(ntok) if ntok is not None else [N] * B
        xf, tcid = _clustered_rows(B, N, Dt, nt, "probe.xf", 3.0)
        emb = synth.uniform_pm1((B, D), "probe.emb", S)
        length = torch.tensor(list(lengths))
        _INP[key] = dict(h=h, xf=xf, emb=emb, length=length, ntok=nt, cid=cid, tcid=tcid, sc=style_rows(sd, eph, emb),
                         mask=R.src_mask(S, length), S=S, N=N, B=B)
    return _INP[key]


def legacy_inputs(B, S, N):
    """The inputs of tests/test_blocks_gpu.py::_setup without its module: golden weights as they are, uniform rows."""
    _, meta = load_golden("fwd_small_dims")
    sd, eph, proj, mcfg = golden_state(meta)
    synth = pkg("synth")
    D, Dt = 512, 256
    h = synth.uniform_pm1((B, S, D), "blk.h", S) * 1.5
    emb = synth.uniform_pm1((B, D), "blk.emb", S)
    xf = synth.uniform_pm1((B, N, Dt), "blk.xf", N) * 1.7
    return (sd, eph, proj, 4, D, Dt, meta), dict(h=h, xf=xf, emb=emb, S=S, N=N, B=B, ntok=[N] * B)


def with_lengths(inp, lengths):
    out = dict(inp)
    out["length"] = torch.tensor(list(lengths))
    out["mask"] = R.src_mask(inp["S"], out["length"])
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the oracle of each entry point (per-sample token counts: every sample alone with exactly its own tokens)
# ------------------------------------------------------------------------------------------------------------------------
def ref_performer(fx, inp, which):
    sd, eph, proj, H = fx[:4]
    slot = ("local", "global")[which]
    with torch.no_grad():
        return R.performer_self_attention(inp["h"], inp["emb"], inp["mask"], sd, f"{PRE}.dual_self_attn.{slot}_attn", H,
                                          eph[f"low.0.{slot}_style"], proj[f"low.0.{slot}"])


def ref_dual(fx, inp):
    sd, eph, proj, H = fx[:4]
    with torch.no_grad():
        return R.dual_self_attention(inp["h"], inp["emb"], inp["mask"], sd, PRE + ".dual_self_attn", H, eph, proj, "low.0")


def dual_base(fx, inp):
    """The dual block with both Performer branches switched off: post_norm(skip + 0.1 pre_norm(x)).  What the attention adds to
    the block's output is measured against this (the block has no residual of its own to subtract)."""
    sd = fx[0]
    p = PRE + ".dual_self_attn"
    with torch.no_grad():
        return R._ln(F.gelu(_LIN(inp["h"], sd, p + ".skip_proj.0")) + 0.1 * R._ln(inp["h"], sd, p + ".pre_norm"), sd, p + ".post_norm")


def _per_sample(inp, ntok_fn, fn):
    outs = []
    for b in range(inp["B"]):
        n = inp["ntok"][b] if ntok_fn is None else ntok_fn(inp["ntok"][b], inp["N"])
        sl = slice(b, b + 1)
        outs.append(fn(inp["h"][sl], inp["xf"][sl, :n], inp["emb"][sl]))
    return torch.cat(outs)


def ref_cross(fx, inp, ntok_fn=None):
    sd, eph, proj, H = fx[:4]
    with torch.no_grad():
        return _per_sample(inp, ntok_fn, lambda h, xf, emb: R.gated_cross_attention(h, xf, emb, sd, PRE + ".cross_attn", H,
                                                                                    eph["low.0.cross_style"]))


def ref_sd(fx, inp, ntok_fn=None, rewrite=None):
    sd, eph, proj, H = fx[:4]
    p = PRE + ".sd_cross_attn"
    sd = sd if rewrite is None else rewrite(sd, p, H)
    with torch.no_grad():
        return _per_sample(inp, ntok_fn, lambda h, xf, emb: R.softmax_cross_ffn(h, xf, sd, p, H))


KINDS = ("performer0", "performer1", "dual", "cross", "sd")


def reference(kind, fx, inp):
    return {"performer0": lambda: ref_performer(fx, inp, 0), "performer1": lambda: ref_performer(fx, inp, 1),
            "dual": lambda: ref_dual(fx, inp), "cross": lambda: ref_cross(fx, inp), "sd": lambda: ref_sd(fx, inp)}[kind]()


def base_of(kind, fx, inp):
    return dual_base(fx, inp) if kind == "dual" else inp["h"]


def mutants_of(kind, variant="mid"):
    if kind in ("performer0", "performer1", "dual"):
        return [n for n in PERFORMER_MUTANTS if variant == "clamp" or n not in CLAMP_ONLY]
    return list(XATTN_MUTANTS if kind == "cross" else SD_MUTANTS)


def mutant(kind, name, fx, inp):
    if kind in ("performer0", "performer1", "dual"):
        with oracle_with(fast_attention=PERFORMER_MUTANTS[name]):
            return reference(kind, fx, inp)
    if kind == "cross":
        state, ntok_fn = XATTN_MUTANTS[name]
        with oracle_with(**({"linear_cross_text_state": state} if state else {})):
            return ref_cross(fx, inp, ntok_fn)
    rewrite, ntok_fn = SD_MUTANTS[name]
    return ref_sd(fx, inp, ntok_fn, rewrite)


# ------------------------------------------------------------------------------------------------------------------------
# metrics over the valid frames
# ------------------------------------------------------------------------------------------------------------------------
def metrics(out, ref, base, length, H):
    """(whole, branch, blockwise) over frames < length[b]: rel_inf of the tensor; rel_inf of (out - base) against (ref - base);
    the worst of that per (sample, block of D / H columns), so that one wrong head of one ragged sample is not averaged away."""
    out, ref, base = out.double(), ref.double(), base.double()
    B, S, D = ref.shape
    valid = torch.arange(S)[None, :] < length[:, None]
    if not valid.any():
        return 0.0, 0.0, 0.0
    d = (out - ref).abs() * valid[..., None]
    br = (ref - base).abs() * valid[..., None]
    whole = float(d.max() / (ref.abs() * valid[..., None]).max().clamp_min(1e-30))
    branch = float(d.max() / br.max().clamp_min(1e-30))
    db = d.view(B, S, H, D // H).amax((1, 3))
    bb = br.view(B, S, H, D // H).amax((1, 3))
    has = length[:, None].expand(B, H) > 0
    blockwise = float((db / bb.clamp_min(1e-30))[has].max())
    return whole, branch, blockwise


def check_past_length(out, ref, length, tol):
    """Rows at or past a sample's length: finite wherever the oracle's are, and for a sample without any valid frame (every key
    masked) the oracle's all-masked result."""
    past = torch.arange(ref.shape[1])[None, :] >= length[:, None]
    fin = torch.isfinite(ref).all(-1) & past
    assert torch.isfinite(out[fin]).all(), "non-finite rows past the length"
    for b in (length == 0).nonzero().flatten().tolist():
        err = float((out[b].double() - ref[b].double()).abs().max() / ref[b].double().abs().max())
        assert err < tol, f"sample {b} (length 0): {err:.2e} against the oracle's all-masked result"


# ------------------------------------------------------------------------------------------------------------------------
# the oracle with a rounding hook
# ------------------------------------------------------------------------------------------------------------------------
def _split3(t):
    hi = t.bfloat16().float()
    return hi + (t - hi).bfloat16().float()


ROUND = {1: lambda t: t.bfloat16().float(), 2: lambda t: t.half().float(), 3: _split3, 4: _split3}
# Linears whose output rows the 16-bit modes store in 16 bits (tensors that only a GEMM or an attention
# core reads): q | k | v rows, the proj_out hidden and output rows, the 4x FFN's hidden rows
_ROUNDED_OUT = (".query", ".key", ".value", ".proj_out.0", ".proj_out.3", ".ffn.1")


@contextlib.contextmanager
def rounding(precision):
    """The oracle computing what DESIGN.md says mode `precision` holds in 16 bits: MFMA operands (the rows that enter a Linear
    and its weights; the (scale | shift) Linear of a stylization runs on the host in fp32 and is left alone), the output rows
    listed above, the Performer core's on-chip images, the text state of the linear cross-attention.  Modes 3 / 4: the bf16
    hi + lo split; mode 4 runs the 4x FFN in fp16.  The text-side key / value Linears are bf16 hi + lo in every mode (DESIGN.md
    section 3: the text caches are fp32-grade)."""
    r = ROUND[precision]

    def lin(x, sd, prefix):
        if ".emb_layers." in prefix:
            return _LIN(x, sd, prefix)
        if "cross_attn" in prefix and prefix.endswith((".key", ".value")):  # the text caches: bf16x3 in every mode, fp32 rows
            return F.linear(_split3(x), _split3(sd[prefix + ".weight"]), sd[prefix + ".bias"])
        rr = ROUND[2] if precision == 4 and ".ffn." in prefix else r
        y = F.linear(rr(x), rr(sd[prefix + ".weight"]), sd[prefix + ".bias"])
        return rr(y) if prefix.endswith(_ROUNDED_OUT) else y

    def fa(*a):
        return fast_attention_variant(*a, rnd=r)

    def state(*a):
        return r(_STATE(*a))

    with oracle_with(_lin=lin, fast_attention=fa, linear_cross_text_state=state):
        yield


def logit_stats(fx, inp):
    """(max |logit|, share of the logits beyond +-15) of the feature maps of both Performers on these inputs."""
    seen = []

    def fa(*a):
        return fast_attention_variant(*a, record=lambda zq, zk: seen.append(zq))

    with oracle_with(fast_attention=fa):
        ref_dual(fx, inp)
    z = torch.cat([s.flatten() for s in seen]).abs()
    return float(z.max()), float((z > 15).float().mean())


# ------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_attention_selective_gpu.py (and of the power proof)
# ------------------------------------------------------------------------------------------------------------------------
# (S, lengths): per launch a full, an S - 1, a tile-edge (33 / 32 / 31, 17 / 16 / 15) and a one-frame sample, and in all but one
# an empty one.  The one-frame sample is in EVERY case on purpose: one key more or less among 15 ... 36 moves the branch by
# 1e-1 ... 2.5e-1, under 4 bf16 tolerances, while among one it replaces the result -- that sample carries length +- 1 and
# rounded-up-to-16 at bf16
SELF_CASES = [(224, (224, 223, 33, 1, 0)), (196, (196, 195, 32, 1, 0)), (98, (98, 97, 31, 16, 1)), (37, (37, 36, 17, 1, 0)),
              (17, (17, 16, 15, 1, 0)), (5, (5, 4, 1, 0))]
CLAMP_CASES = [(196, (196, 195, 17, 1, 0)), (37, (37, 36, 17, 1, 0))]
BIG_CASES = [(98, (98, 97, 33, 16, 0)), (17, (17, 16, 15, 1, 0))]
# (S, lengths, N, token counts): N on both sides of the fold limit (64), of the 96-column softmax core and of the 32-token steps
TEXT_CASES = [(98, (98, 97, 17), 1, (1, 1, 1)), (37, (37, 36, 17), 6, (6, 5, 1)), (98, (98, 97, 17), 28, (28, 27, 1)),
              (196, (196, 195, 17), 64, (64, 63, 1)), (98, (98, 97, 17), 65, (65, 64, 1)), (196, (196, 195, 17), 85, (85, 84, 1)),
              (37, (37, 36, 17), 96, (96, 95, 1)), (98, (98, 97, 17), 128, (128, 127, 1))]

# Branch tolerances.  MEASURED[kind group, variant][precision] is the worst blockwise branch error, over the cases above, of the
# oracle under rounding(precision) against the plain oracle (tests/test_attention_probe_host.py re-measures it); the tolerance
# is 4 x that: the margin covers accumulation order and the roundings the hook does not model.  No figure here comes from a
# kernel.  (The blockwise metric bounds the branch metric from above, so one table gates both.)
MEASURED = {
    ("performer", "mid"): {3: 1.6e-05, 4: 1.6e-05, 2: 1.3e-03, 1: 9.9e-03},
    ("dual", "mid"): {3: 2.6e-05, 4: 2.6e-05, 2: 2.1e-03, 1: 1.7e-02},
    ("performer", "clamp"): {3: 3.8e-05, 4: 3.8e-05, 1: 2.7e-02},
    ("dual", "clamp"): {3: 3.5e-05, 4: 3.5e-05, 1: 2.2e-02},
    ("cross", "mid"): {3: 6.1e-05, 4: 6.1e-05, 2: 4.2e-03, 1: 4.8e-02},
    ("sd", "mid"): {3: 2.0e-05, 4: 4.6e-04, 2: 1.8e-03, 1: 1.3e-02},
    ("performer256", "mid"): {3: 1.4e-05, 4: 1.4e-05, 2: 1.0e-03, 1: 7.9e-03},
}
# Mutants whose distance from the oracle is below POWER x the bf16 tolerance in at least one case (the host test asserts that
# each one listed really is): mode 1 does not claim them; every other mode the group runs sees them at >= POWER x its tolerance.
# The denominator is a per-row factor in front of a LayerNorm, which removes it up to the LayerNorm's eps: its mutant moves the
# branch by 5e-2 ... 1.5e-1 whatever the inputs (0.5 ... 1.4 bf16 tolerances; 4.9 at head_dim 256).  Length +- 1 and rounded up
# to 16 are claimed at bf16 by the `mid` fixture in every case (its one-frame sample); on the `clamp` fixture, whose bf16
# tolerance is 2.7 x wider, length + 1 stays at 1.2 ... 2.7, and the clamp itself at 3.0 on the Performer entry (5.3 on the
# dual block, which claims it).  One text token more among 5 ... 127 moves the linear cross-attention by 2.4 bf16 tolerances.
BF16_OUT_OF_REACH = {
    ("performer", "mid"): ("textbook denominator",),
    ("dual", "mid"): ("textbook denominator",),
    ("performer", "clamp"): ("length + 1", "textbook denominator", "clamp removed"),
    ("dual", "clamp"): ("length + 1", "textbook denominator"),
    ("cross", "mid"): ("token count + 1",),
    ("sd", "mid"): (),
    ("performer256", "mid"): (),
}
MARGIN = 4.0


def group_of(kind):
    return "performer" if kind.startswith("performer") else kind


def branch_tol(kind, variant, precision, width="small"):
    return MARGIN * MEASURED[group_of(kind) + ("256" if width == "big" else ""), variant][precision]


def measure_rounding(kind, fx, inp, precision):
    ref = reference(kind, fx, inp)
    with rounding(precision):
        got = reference(kind, fx, inp)
    return metrics(got, ref, base_of(kind, fx, inp), inp["length"], fx[3])
