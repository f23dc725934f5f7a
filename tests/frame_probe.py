"""Probe fixtures for the step outside the decoder layers (the "frame"): the stem (time chain, text half, gated mix, post_mlp,
the 8L (scale | shift) rows), the per-loop stem cache, the text cache, joint_embed + sequence_embedding, the `down` Conv-as-Linear
with the halved lengths, the `up` Linear with the U's skip, and the output head.  Same method as tests/attention_probe.py: the
pieces of the oracle (oracle/denoiser_ref.py) restated with switches, deliberately wrong variants ("mutants") of each, a rounding
hook from which the tolerances of tests/test_frame_selective_gpu.py are measured, and the metric of each stage.

CPU only; nothing of the package is imported but `synth`.  tests/test_frame_probe_host.py asserts that the restated pieces equal
the oracle bit for bit with every switch off, re-measures MEASURED, and proves from the oracle alone that every mutant is at
least POWER x MARGIN x MEASURED away from the truth in its stage's metric.

Stages and what each is read through:
  stem        emb and the 8L (scale | shift) rows of mdm_stem_embeddings; rel_inf per (slot, sample) row, worst row
  stem_cache  the time table and gx of mdm_stem_cache_build; rel_inf per row, worst row
  embed_down  slot 0 of layer 0 of the trace (the dual block on h_low under the coarse mask), given the (scale | shift) rows;
              the worst (sample, head block) branch error of attention_probe.metrics over the valid coarse frames
  block0      the same tensor with nothing given: stem (plain or cached), embedding, down and the dual block in one piece
  stem_pair   the same tensor of a forward on the plain stem against that of a forward on a stem cache; same metric
  up_skip     slot 0 of layer L of the trace, given the last coarse block and the (scale | shift) rows; same metric, fine frames
  head        the output given the last block; rel_inf per sample over all T frames
  text_cache  lin_at (held transposed: A^T) / sd_k / sd_v of every layer; rel_inf per (layer, sample), sd_k / sd_v over a sample's own tokens only
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from conftest import golden_state, load_golden, pkg

import attention_probe as AP

R = AP.R
POWER, MARGIN = AP.POWER, AP.MARGIN  # the project's conditions (tests/attention_probe.py)

WIDTHS = {"small": "fwd_small_dims", "big": "fwd_big_dims", "tools": "fwd_tools_shape", "tiny": "fwd_tiny_eqdim"}
PRECISIONS = {"small": (3, 4, 2, 1), "big": (3, 4, 2, 1), "tools": (3, 4, 2, 1), "tiny": (3, 1)}
FRAME_WIDTHS = ("small", "big", "tools")  # `tiny` (D = Dt = 64: no text_proj) serves the stem alone

# Gains on the seeded weights, where a term would otherwise hide inside a tolerance:
#   STYLE_GAIN   on out_layers.2 of both Performers' stylizations of layer 0 of both scales (as attention_probe does): the
#                attention branch is the only reader of the coarse / fine mask in the dual block that the embed_down and up_skip
#                stages are read through; at the seeded 0.1 x 0.1 of the residual a wrong halved length is 1e-3 of the tensor
#   SEQ_GAIN     sequence_embedding is U(-1, 1) against joint_embed rows of variance 1: after the k = 2 `down` and two
#                LayerNorms a wrong row is a third of the signal; x 3 makes it the larger half, so that every sequence_embedding
#                mutant is far away at the shortest case (T = 2, where "m mod T / 2" and "shifted" move one row each)
#   UPB_GAIN     upsample.bias is U(-0.1, 0.1) (fan-in init) against up(h) + skip rows of size 2: 1e-3 of the row energy
#   OUTB_GAIN    out.bias is U(-0.1, 0.1) against output rows of several units: under the fp16 noise of a K = D head
STYLE_GAIN = AP.STYLE_GAIN
SEQ_GAIN, UPB_GAIN, OUTB_GAIN = 3.0, 30.0, 30.0

_FIX, _FIX64 = {}, {}


def frame_state(width):
    """dict(sd, eph, proj, H, D, Dt, L, E, meta) of a golden case with the gains above.  Memoised; read-only."""
    if width not in _FIX:
        _, meta = load_golden(WIDTHS[width])
        sd, eph, proj, mcfg = golden_state(meta)
        for scale in ("low", "high"):
            for slot in ("local", "global"):
                p = f"decoder_blocks_{scale}.0.module.dual_self_attn.{slot}_attn.style_block.out_layers.2"
                sd[p + ".weight"], sd[p + ".bias"] = sd[p + ".weight"] * STYLE_GAIN, sd[p + ".bias"] * STYLE_GAIN
        sd["sequence_embedding"] = sd["sequence_embedding"] * SEQ_GAIN
        sd["upsample.bias"] = sd["upsample.bias"] * UPB_GAIN
        sd["out.bias"] = sd["out.bias"] * OUTB_GAIN
        _FIX[width] = dict(sd=sd, eph=eph, proj=proj, H=mcfg["num_heads"], D=mcfg["latent_dim"], Dt=meta["text_latent_dim"],
                           L=mcfg["num_layers"], E=mcfg["moe_num_experts"], meta=meta, width=width)
    return _FIX[width]


def as64(fs):
    """The same fixture in float64 (the reference of the stem, head and text-cache stages)."""
    w = fs["width"]
    if w not in _FIX64:
        out = dict(fs)
        out["sd"] = {k: v.double() if v.is_floating_point() else v for k, v in fs["sd"].items()}
        out["eph"] = {k: (a.double(), b.double()) for k, (a, b) in fs["eph"].items()}
        out["proj"] = {k: v.double() for k, v in fs["proj"].items()}
        _FIX64[w] = out
    return _FIX64[w]


# ------------------------------------------------------------------------------------------------------------------------
# the rounding hook
# ------------------------------------------------------------------------------------------------------------------------
_ID = lambda t: t


class _Q:
    """What the restated pieces round: `chain` the operands of the time / text chains, `r` the operands of the Linears that run
    in the mode's format, `store` a tensor the mode keeps as 16-bit rows, `x3` the operands of a Linear that is bf16x3 in every
    mode, `ulp` whether the sinusoid's frequencies are one fp32 ulp off."""
    def __init__(self):
        self.chain = self.r = self.store = self.x3 = _ID
        self.ulp = False


_CUR = _Q()


def _r(fn, t):
    return t if fn is _ID else fn(t.float()).to(t.dtype)


@contextlib.contextmanager
def frame_rounding(precision, acts16=True, single_pass_chain=False, ulp=True):
    """attention_probe.rounding(precision) extended to what the code holds in 16 bits outside the layers, read out of
    csrc/model.hip (stem_time_branch, stem_text_branch, stem_embeddings, mdm_denoiser_forward) and packing.py (_ALWAYS_X3):

      * joint_embed reads the fp32 motion rows with bf16 hi + lo weights in every mode (`cj.prec = 3`): bf16x3.
      * down, up and out are Linears of the mode: in modes 1 / 2 on the 16-bit shadows (h016, xa16, xb16) with single-plane
        weights of the mode's format; in modes 3 / 4 bf16x3 on fp32 rows.
      * The time chain (sinusoid -> learnable_time_embed -> time_embed -> time_proj -> proj_time) and the text half
        ([text_proj] -> proj_text) read fp32 rows and _ALWAYS_X3 weights with prec = 3 in every mode, in the plain stem
        (stem_embeddings' `c3`) as in the table and gx of the stem cache (mdm_stem_cache_build): bf16x3.  (Until this probe
        the plain stem ran them at the run's `prec`: in modes 1 AND 2 a single pass on the bf16 hi plane, activations rounded
        to bf16 as well -- an fp16 run has no fp16 image of these weights.  `single_pass_chain=True` is that arithmetic;
        tests/test_frame_probe_host.py::test_the_single_pass_chain_was_too_coarse_for_the_fp16_mode holds the figures quoted
        for it: mode 2 measured 5.3e-3 where it now measures 7e-4, timestep +- 1 under 4 fp16 tolerances on fwd_tools_shape.)
      * mix (to_bf16 / the 16-bit store of gated_mix_gather), the post_mlp hidden rows (linear_to_act), emb's 16-bit copy and
        the e1 rows are 16-bit rows of the mode's format in modes 1 / 2; post_mlp, style_eph and style_emb are Linears of the mode.
      * `acts16=False`: a model whose widths are no multiple of 64 (fwd_tiny_eqdim) keeps fp32 rows in mode 1; every Linear is
        then a single bf16 pass on them.
      * The device evaluates expf / cosf / sinf itself: the sinusoid's frequencies are taken one fp32 ulp off (alternating), which
        moves the argument t f by up to 1e-4 at t = 999.  This is an allowance for the device's expf, not a rounding of something
        the code holds in 16 bits; `ulp=False` leaves it out, and SINUSOID_ULP_SHARE records how much of the fp32-grade figures
        of the stem and the stem cache it is (the host test prints and asserts both).

    The decoder blocks below are under attention_probe.rounding(precision) as before."""
    global _CUR
    q = _Q()
    r16 = AP.ROUND[precision]
    q.x3 = AP._split3
    q.r = r16
    q.chain = AP.ROUND[1] if (single_pass_chain and precision in (1, 2)) else AP._split3
    q.store = r16 if (precision in (1, 2) and acts16) else _ID
    q.ulp = ulp
    old, _CUR = _CUR, q
    try:
        with AP.rounding(precision):
            yield
    finally:
        _CUR = old


def _linq(x, w, b, fn):
    return F.linear(_r(fn, x), _r(fn, w), b)


# ------------------------------------------------------------------------------------------------------------------------
# the stem, restated (oracle fused_embedding + the per-slot Linears of stylization) with switches
# ------------------------------------------------------------------------------------------------------------------------
def sinusoid(ts, dim, swap=False):
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
    if _CUR.ulp:
        up = torch.nextafter(freqs, torch.full_like(freqs, 2.0))
        dn = torch.nextafter(freqs, torch.zeros_like(freqs))
        freqs = torch.where(torch.arange(half) % 2 == 0, up, dn)
        freqs[0] = 1.0  # expf(0) is exact
    args = ts[:, None].float() * freqs[None]
    return torch.cat([torch.sin(args), torch.cos(args)] if swap else [torch.cos(args), torch.sin(args)], dim=-1)


def slot_prefixes(L):
    """(state-dict prefix of the stylization, ephemeral name) of the 8L (scale | shift) slots, in the order of `sc`."""
    out = []
    for scale in ("low", "high"):
        for i in range(L):
            pre = f"decoder_blocks_{scale}.{i}.module"
            for slot, sub in (("local_style", ".dual_self_attn.local_attn.style_block"),
                              ("global_style", ".dual_self_attn.global_attn.style_block"),
                              ("cross_style", ".cross_attn.base_ca.proj_out"), ("ffn_style", ".ffn.proj_out")):
                out.append((pre + sub, f"{scale}.{i}.{slot}"))
    return out


def proj_time(fs, ts, swap=False):
    """gated_fusion.proj_time(time_proj(time_embed(learnable_time_embed(sinusoid(t))))): a row of the stem cache's table."""
    sd, q = fs["sd"], _CUR
    lin = lambda x, p: _linq(x, sd[p + ".weight"], sd[p + ".bias"], q.chain)
    te = sinusoid(ts, fs["D"], swap).to(sd["time_proj.weight"].dtype)
    te = lin(F.silu(lin(te, "learnable_time_embed.mlp.0")), "learnable_time_embed.mlp.2")
    te = lin(F.silu(lin(te, "time_embed.0")), "time_embed.2")
    te = lin(te, "time_proj")
    return lin(te, "gated_fusion.proj_time")


def proj_text(fs, xp, skip_text_proj=False):
    """gated_fusion.proj_text([text_proj](xf_proj)): a row of the stem cache's gx."""
    sd, q = fs["sd"], _CUR
    xp = xp.to(sd["time_proj.weight"].dtype)
    if xp.shape[-1] != fs["D"]:
        if skip_text_proj:
            xp = F.pad(xp, (0, fs["D"] - xp.shape[-1]))
        else:
            w, b = fs["eph"]["text_proj"]
            xp = _linq(xp, w, b, q.chain)
    return _linq(xp, sd["gated_fusion.proj_text.weight"], sd["gated_fusion.proj_text.bias"], q.chain)


def stem_from(fs, t, x, gate_swapped=False):
    """(emb (B, D), sc (8L, B, 2D)) from the two halves of the gate."""
    sd, q = fs["sd"], _CUR
    g = torch.sigmoid(t + x)
    fused = g * x + (1 - g) * t if gate_swapped else g * t + (1 - g) * x
    fused = _r(q.store, fused)
    hid = _r(q.store, F.silu(_linq(fused, sd["gated_fusion.post_mlp.0.weight"], sd["gated_fusion.post_mlp.0.bias"], q.r)))
    emb = _linq(hid, sd["gated_fusion.post_mlp.2.weight"], sd["gated_fusion.post_mlp.2.bias"], q.r)
    e16 = _r(q.store, emb)
    sc = []
    for pre, name in slot_prefixes(fs["L"]):
        w, b = fs["eph"][name]
        e1 = _r(q.store, F.silu(_linq(e16, w, b, q.r)))
        sc.append(_linq(e1, sd[pre + ".emb_layers.1.weight"], sd[pre + ".emb_layers.1.bias"], q.r))
    return emb, torch.stack(sc)


def _swap_layers(sc):
    """(8L, B, 2D) with the four slots of layers (0, 1), (2, 3), ... exchanged (L even: fwd_tools_shape)."""
    return sc.view(sc.shape[0] // 8, 2, 4, *sc.shape[1:]).flip(1).reshape(sc.shape)


# name -> (fn(fs, ts, xp) -> (emb, sc), applies(fs, B))
STEM_MUTANTS = {
    "timestep + 1": (lambda fs, ts, xp: stem_from(fs, proj_time(fs, ts + 1), proj_text(fs, xp)), lambda fs, B: True),
    "timestep - 1": (lambda fs, ts, xp: stem_from(fs, proj_time(fs, ts - 1), proj_text(fs, xp)), lambda fs, B: True),
    "cos and sin halves swapped": (lambda fs, ts, xp: stem_from(fs, proj_time(fs, ts, swap=True), proj_text(fs, xp)),
                                   lambda fs, B: True),
    "time and text swapped in the gate": (lambda fs, ts, xp: stem_from(fs, proj_time(fs, ts), proj_text(fs, xp), gate_swapped=True),
                                          lambda fs, B: True),
    # possible only where a text_proj exists (Dt != D); the Dt columns then enter proj_text directly, zero-padded to D
    "text_proj skipped": (lambda fs, ts, xp: stem_from(fs, proj_time(fs, ts), proj_text(fs, xp, skip_text_proj=True)),
                          lambda fs, B: fs["Dt"] != fs["D"]),
    "sample rows rolled by one": (lambda fs, ts, xp: tuple(a.roll(1, d) for a, d in zip(stem(fs, ts, xp), (0, 1))),
                                  lambda fs, B: B > 1),
    "slot j delivered in slot j + 1": (lambda fs, ts, xp: (lambda e, s: (e, s.roll(1, 0)))(*stem(fs, ts, xp)), lambda fs, B: True),
    "scale and shift halves swapped": (lambda fs, ts, xp: (lambda e, s: (e, s.roll(fs["D"], -1)))(*stem(fs, ts, xp)),
                                       lambda fs, B: True),
    "slots of layer i swapped with layer i + 1": (lambda fs, ts, xp: (lambda e, s: (e, _swap_layers(s)))(*stem(fs, ts, xp)),
                                                  lambda fs, B: fs["L"] == 2),
}
# the stem cache: name -> fn(fs, steps, xp) -> (table, gx)
CACHE_MUTANTS = {
    "timestep + 1": lambda fs, steps, xp: (proj_time(fs, torch.arange(steps) + 1), proj_text(fs, xp)),
    "timestep - 1": lambda fs, steps, xp: (proj_time(fs, torch.arange(steps) - 1), proj_text(fs, xp)),
    "cos and sin halves swapped": lambda fs, steps, xp: (proj_time(fs, torch.arange(steps), swap=True), proj_text(fs, xp)),
    "text_proj skipped": lambda fs, steps, xp: (proj_time(fs, torch.arange(steps)), proj_text(fs, xp, skip_text_proj=True)),
    "sample rows rolled by one": lambda fs, steps, xp: (proj_time(fs, torch.arange(steps)), proj_text(fs, xp).roll(1, 0)),
    "last partial chunk not written": lambda fs, steps, xp: (_zero_tail(proj_time(fs, torch.arange(steps)), steps // 128 * 128),
                                                              _zero_tail(proj_text(fs, xp), xp.shape[0] // 128 * 128)),
}


def _zero_tail(t, n):
    t = t.clone()
    t[n:] = 0
    return t


def stem(fs, ts, xp):
    return stem_from(fs, proj_time(fs, ts), proj_text(fs, xp))


def stem_cache(fs, steps, xp):
    return proj_time(fs, torch.arange(steps)), proj_text(fs, xp)


def rows_rel(out, ref):
    """rel_inf per row (last axis), worst row: one wrong slot of 8L or one wrong sample of 130 is not averaged away."""
    out, ref = out.double(), ref.double()
    return float(((out - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-30)).max())


def stem_metric(got, ref):
    return max(rows_rel(got[0], ref[0]), rows_rel(got[1], ref[1]))


STEM_BATCHES = (1, 3, 33, 130)
STEM_CACHE_STEPS = {"small": 300, "tools": 300, "big": 130}
STEM_CACHE_BATCH = 130


def stem_inputs(width, B):
    """Timesteps with 0, 1, 998, 999 and a repeated value (B = 1: 999 alone), text rows of unit variance."""
    fs = frame_state(width)
    ts = torch.tensor(([999, 0, 1, 998, 500, 500] + [(37 * i + 11) % 1000 for i in range(B)])[:B])
    xp = pkg("synth").uniform_pm1((B, fs["Dt"]), "frame.xp", B) * (3.0 ** 0.5)
    return ts, xp


# ------------------------------------------------------------------------------------------------------------------------
# the frame around the layers, restated (oracle denoiser_forward) with switches
# ------------------------------------------------------------------------------------------------------------------------
def embed(fs, x, seq="true"):
    """h = joint_embed(x) + sequence_embedding[:T]."""
    sd, q = fs["sd"], _CUR
    B, T, _ = x.shape
    se = sd["sequence_embedding"]
    rows = {"true": lambda: se[None, :T, :], "shifted": lambda: se.roll(1, 0)[None, :T, :],
            "mod_half": lambda: se[torch.arange(T) % (T // 2)][None],
            "sample0": lambda: se[None, :T, :] * (torch.arange(B) == 0).to(se.dtype)[:, None, None]}[seq]()
    return _linq(x.to(se.dtype), sd["joint_embed.weight"], sd["joint_embed.bias"], q.x3) + rows


def down(fs, h, pairs_shifted=False, taps_swapped=False):
    sd, q = fs["sd"], _CUR
    w = sd["downsample.weight"]
    h = _r(q.r, _r(q.store, h))
    if pairs_shifted:  # frame pairs (2i + 1, 2i + 2)
        h = h.roll(-1, 1)
    return F.conv1d(h.permute(0, 2, 1), _r(q.r, w.flip(-1) if taps_swapped else w), sd["downsample.bias"], stride=2).permute(0, 2, 1)


LEN_LOW = {"floor": lambda n: (n / 2).long(), "ceil": lambda n: (n + 1) // 2, "same": lambda n: n}


def up_skip(fs, x_low, h, taps_swapped=False, bias="all", skip=1.0, skip_without_seq=False):
    sd, q = fs["sd"], _CUR
    w = sd["upsample.weight"]
    xl = _r(q.r, _r(q.store, x_low)).permute(0, 2, 1)
    w = _r(q.r, w.flip(-1) if taps_swapped else w)
    if bias == "all":
        h_up = F.conv_transpose1d(xl, w, sd["upsample.bias"], stride=2).permute(0, 2, 1)
    else:  # on the even fine frames only
        h_up = F.conv_transpose1d(xl, w, None, stride=2).permute(0, 2, 1)
        h_up[:, 0::2] += sd["upsample.bias"]
    if skip_without_seq:
        h = h - sd["sequence_embedding"][None, :h.shape[1], :]
    if skip == 0.0:
        return h_up
    return h_up + h if skip == 1.0 else h_up + skip * h


def head(fs, hc, bias=True, ragged_zero=False, rolled=False):
    sd, q = fs["sd"], _CUR
    y = F.linear(_r(q.r, _r(q.store, hc.to(sd["out.weight"].dtype))), _r(q.r, sd["out.weight"]), sd["out.bias"] if bias else None)
    if ragged_zero:  # the ragged tile of N = 263
        y = y.clone()
        y[..., 256:] = 0
    if rolled:
        y = y.reshape(-1, y.shape[-1]).roll(1, 0).reshape(y.shape)
    return y


def dual_prefix(scale):
    return f"decoder_blocks_{scale}.0.module.dual_self_attn"


def dual_given_rows(fs, h, length, scale, sc_local, sc_global):
    """The oracle's dual block of layer 0 of `scale` on h, with the two Performers' (scale | shift) rows GIVEN (the device's own,
    or the stem's): R.stylization with its emb Linears replaced by the rows."""
    sd = fs["sd"]
    p = dual_prefix(scale)
    rows = {p + ".local_attn.style_block": sc_local, p + ".global_attn.style_block": sc_global}

    def sty(x, emb, sd_, prefix, eph_wb):
        eo = rows[prefix].to(x.dtype).unsqueeze(1)
        D = x.shape[-1]
        y = R._ln(x, sd_, prefix + ".norm") * (1 + eo[..., :D]) + eo[..., D:]
        return R._lin(F.silu(y), sd_, prefix + ".out_layers.2")

    tag = f"{scale}.0"
    with AP.oracle_with(stylization=sty), torch.no_grad():
        return R.dual_self_attention(h, None, R.src_mask(h.shape[1], length), sd, p, fs["H"],
                                     {tag + ".local_style": None, tag + ".global_style": None}, fs["proj"], tag)


def dual_base(fs, h, scale):
    """The dual block with both Performer branches off (attention_probe.dual_base for either scale)."""
    sd, p = fs["sd"], dual_prefix(scale)
    with torch.no_grad():
        return R._ln(F.gelu(AP._LIN(h, sd, p + ".skip_proj.0")) + 0.1 * R._ln(h, sd, p + ".pre_norm"), sd, p + ".post_norm")


def sc_slot(fs, scale, which):
    return (0 if scale == "low" else 4 * fs["L"]) + which


def branch_metric(fs, out, ref, base, length):
    return AP.metrics(out, ref, base, length, fs["H"])


def per_sample_rel(out, ref):
    out, ref = out.double(), ref.double()
    B = ref.shape[0]
    return float(((out - ref).abs().reshape(B, -1).amax(1) / ref.abs().reshape(B, -1).amax(1).clamp_min(1e-30)).max())


# (B, T, lengths): T / 2 odd in all but the last, B T / 2 never a multiple of 16, odd lengths (the halved length rounds down), an
# empty and a one-frame sample, and in the last case the last row of sequence_embedding
CASES = [(3, 2, (2, 1, 0)), (3, 6, (6, 5, 1)), (3, 14, (14, 13, 3)), (5, 34, (34, 33, 17, 1, 0)), (2, 66, (66, 31)), (2, 196, (196, 195))]
BIG_CASES = [CASES[1], CASES[3], CASES[4]]


def cases_of(width):
    return BIG_CASES if width == "big" else CASES


_INP = {}


def frame_inputs(width, case, ts=None):
    """Memoised inputs and oracle intermediates of one case: x, timesteps, text row, lengths; the oracle's emb, (scale | shift)
    rows, h_embed, h_low and the two readouts.  `x_low` stands for the last coarse block's output in the host proofs (on the
    GPU that tensor is the device's own): the oracle's layer-0 dual block of h_low, a tensor of the right statistics."""
    key = (width, case, None if ts is None else tuple(ts.tolist()))
    if key not in _INP:
        fs = frame_state(width)
        B, T, lengths = case
        synth = pkg("synth")
        x = synth.uniform_pm1((B, T, 263), "frame.x", T) * (3.0 ** 0.5)
        ts0, xp = stem_inputs(width, B)
        ts = ts0 if ts is None else ts
        length = torch.tensor(list(lengths))
        with torch.no_grad():
            emb, sc = stem(fs, ts, xp)
            h = embed(fs, x)
            h_low = down(fs, h)
            len_low = LEN_LOW["floor"](length)
            lo = dual_given_rows(fs, h_low, len_low, "low", sc[sc_slot(fs, "low", 0)], sc[sc_slot(fs, "low", 1)])
            hc = up_skip(fs, lo, h)
            hi = dual_given_rows(fs, hc, length, "high", sc[sc_slot(fs, "high", 0)], sc[sc_slot(fs, "high", 1)])
        _INP[key] = dict(x=x, ts=ts, xp=xp, length=length, len_low=len_low, emb=emb, sc=sc, h=h, h_low=h_low, lo=lo, x_low=lo,
                         hc=hc, hi=hi, base_lo=dual_base(fs, h_low, "low"), base_hi=dual_base(fs, hc, "high"), B=B, T=T)
    return _INP[key]


def read_low(fs, inp, h_low, len_low=None, sc=None):
    sc = inp["sc"] if sc is None else sc
    return dual_given_rows(fs, h_low, inp["len_low"] if len_low is None else len_low, "low", sc[sc_slot(fs, "low", 0)],
                           sc[sc_slot(fs, "low", 1)])


def read_high(fs, inp, hc, sc=None):
    sc = inp["sc"] if sc is None else sc
    return dual_given_rows(fs, hc, inp["length"], "high", sc[sc_slot(fs, "high", 0)], sc[sc_slot(fs, "high", 1)])


def _changes_a_coarse_length(case, changed):
    """A length mutant is exercised by every case with a sample whose coarse length it changes and that has a valid coarse frame
    to read it through (the metric is over the valid frames: a one-frame sample, 0 coarse frames, shows nothing)."""
    return any(n // 2 >= 1 and changed(n) != n // 2 for n in case[2])


# name -> (fn(fs, inp) -> readout of layer low.0, applies(case))
# the step of test_forward_with_and_without_the_stem_cache: per-sample timesteps on the chunk edges of the stem cache's table
PAIR_CASE = (6, 6, (6, 5, 4, 3, 2, 6))


def pair_timesteps(width):
    steps = STEM_CACHE_STEPS[width]
    return torch.tensor([0, 127, 128, 255, 256, steps - 1] if steps > 256 else [0, 1, 127, 128, 129, steps - 1])


def stem_pair(fs, inp, precision):
    """How far apart two correct stems put slot 0 of layer 0, in the block0 metric.  The plain stem and the stem cache run the
    same bf16x3 chains on GEMMs of different heights (B rows; chunks of 128), so their t and x agree to an fp32-grade error
    and no better; behind them mix is stored once in the mode's 16-bit format, and a value near a rounding boundary lands one
    16-bit ulp apart.  Measured as the worst pair among three fp32-grade evaluations of the chains (under the hook's bf16x3, in
    plain fp32, in f64 rounded to fp32), everything behind them under frame_rounding(precision)."""
    fs64 = as64(fs)
    with frame_rounding(precision):
        chains = [(proj_time(fs, inp["ts"]), proj_text(fs, inp["xp"]))]
    chains.append((proj_time(fs, inp["ts"]), proj_text(fs, inp["xp"])))
    chains.append((proj_time(fs64, inp["ts"]).float(), proj_text(fs64, inp["xp"]).float()))
    with frame_rounding(precision):
        h_low = down(fs, embed(fs, inp["x"]))
        outs = [read_low(fs, inp, h_low, sc=stem_from(fs, t, x)[1]) for t, x in chains]
    return max(branch_metric(fs, outs[i], outs[j], inp["base_lo"], inp["len_low"])[2] for i, j in ((0, 1), (0, 2), (1, 2)))


EMBED_MUTANTS = {
    "sequence_embedding shifted by one row": (lambda fs, inp: read_low(fs, inp, down(fs, embed(fs, inp["x"], "shifted"))), lambda c: True),
    "sequence_embedding indexed m mod T / 2": (lambda fs, inp: read_low(fs, inp, down(fs, embed(fs, inp["x"], "mod_half"))), lambda c: True),
    "sequence_embedding added to sample 0 only": (lambda fs, inp: read_low(fs, inp, down(fs, embed(fs, inp["x"], "sample0"))),
                                                  lambda c: any(n >= 2 for n in c[2][1:])),
    "frame pairs (2i + 1, 2i + 2)": (lambda fs, inp: read_low(fs, inp, down(fs, inp["h"], pairs_shifted=True)), lambda c: True),
    "taps of downsample.weight swapped": (lambda fs, inp: read_low(fs, inp, down(fs, inp["h"], taps_swapped=True)), lambda c: True),
    "coarse length ceil(len / 2)": (lambda fs, inp: read_low(fs, inp, inp["h_low"], LEN_LOW["ceil"](inp["length"])),
                                    lambda c: _changes_a_coarse_length(c, lambda n: (n + 1) // 2)),
    "coarse length len": (lambda fs, inp: read_low(fs, inp, inp["h_low"], LEN_LOW["same"](inp["length"])),
                          lambda c: _changes_a_coarse_length(c, lambda n: min(n, c[1] // 2))),
}
UP_MUTANTS = {
    "taps of upsample.weight swapped": lambda fs, inp: read_high(fs, inp, up_skip(fs, inp["x_low"], inp["h"], taps_swapped=True)),
    "upsample.bias on the even frames only": lambda fs, inp: read_high(fs, inp, up_skip(fs, inp["x_low"], inp["h"], bias="even")),
    "skip omitted": lambda fs, inp: read_high(fs, inp, up_skip(fs, inp["x_low"], inp["h"], skip=0.0)),
    "skip doubled": lambda fs, inp: read_high(fs, inp, up_skip(fs, inp["x_low"], inp["h"], skip=2.0)),
    "skip taken before sequence_embedding": lambda fs, inp: read_high(fs, inp, up_skip(fs, inp["x_low"], inp["h"], skip_without_seq=True)),
}
HEAD_MUTANTS = {
    "bias missing": lambda fs, hc: head(fs, hc, bias=False),
    "columns from 256 on zero": lambda fs, hc: head(fs, hc, ragged_zero=True),
    "rows rolled by one": lambda fs, hc: head(fs, hc, rolled=True),
}


# ------------------------------------------------------------------------------------------------------------------------
# the text cache
# ------------------------------------------------------------------------------------------------------------------------
TEXT_N = (1, 6, 33, 85, 128)


def text_inputs(width, N):
    """B = 3 with token counts (N, max(1, N - 1), 1); rows past a count hold junk of 9 x the token scale."""
    fs = frame_state(width)
    synth = pkg("synth")
    ntok = (N, max(1, N - 1), 1)
    xf = synth.uniform_pm1((3, N, fs["Dt"]), "frame.xf", N) * (3.0 ** 0.5)
    junk = synth.uniform_pm1((3, N, fs["Dt"]), "frame.xf.junk", N) * (9.0 * 3.0 ** 0.5)
    past = torch.arange(N)[None, :] >= torch.tensor(ntok)[:, None]
    return torch.where(past[..., None], junk, xf), ntok


def layer_prefixes(L):
    return [f"decoder_blocks_{s}.{i}.module" for s in ("low", "high") for i in range(L)]


def text_state(fs, xf, ntok, ntok_fn=None):
    """(lin_at (2L, B, H, dh, dh), sd_k, sd_v (2L, B, N, D)) of every layer, every sample alone on exactly its own tokens;
    sd_k / sd_v rows past a count are zero here and unspecified on the device."""
    sd, H = fs["sd"], fs["H"]
    B, N, _ = xf.shape
    xf = xf.to(sd["out.weight"].dtype)
    at, ks, vs = [], [], []
    with torch.no_grad():
        for pre in layer_prefixes(fs["L"]):
            a, k, v = [], xf.new_zeros(B, N, fs["D"]), xf.new_zeros(B, N, fs["D"])
            for b in range(B):
                n = ntok[b] if ntok_fn is None else ntok_fn(ntok[b], N)
                a.append(R.linear_cross_text_state(xf[b:b + 1, :n], sd, pre + ".cross_attn.base_ca", H)[0])
                k[b, :ntok[b]] = R._lin(xf[b, :ntok[b]], sd, pre + ".sd_cross_attn.key")
                v[b, :ntok[b]] = R._lin(xf[b, :ntok[b]], sd, pre + ".sd_cross_attn.value")
            at.append(torch.stack(a)), ks.append(k), vs.append(v)
    return torch.stack(at), torch.stack(ks), torch.stack(vs)


def text_metric(got, ref, ntok):
    """Worst rel_inf per (layer, sample) of the three slabs; sd_k / sd_v over the sample's own tokens."""
    worst = 0.0
    L2, B = ref[0].shape[:2]
    for li in range(L2):
        for b in range(B):
            worst = max(worst, rows_rel(got[0][li, b].reshape(1, -1), ref[0][li, b].reshape(1, -1)))
            for s in (1, 2):
                worst = max(worst, rows_rel(got[s][li, b, :ntok[b]].reshape(1, -1), ref[s][li, b, :ntok[b]].reshape(1, -1)))
    return worst


def _text_xattn(name):
    state, ntok_fn = AP.XATTN_MUTANTS[name]

    def fn(fs, xf, ntok):
        with AP.oracle_with(**({"linear_cross_text_state": state} if state else {})):
            return text_state(fs, xf, ntok, ntok_fn)
    return fn


# name -> (fn(fs, xf, ntok) -> slabs, applies(N)); a single token leaves no count to ignore and no softmax axis to mistake
TEXT_MUTANTS = {name: (_text_xattn(name), (lambda N: N > 1) if name.startswith(("token count", "text softmax")) else (lambda N: True))
                for name in AP.XATTN_MUTANTS}
TEXT_MUTANTS["slab of layer j delivered for layer j + 1"] = (
    lambda fs, xf, ntok: tuple(t.roll(1, 0) for t in text_state(fs, xf, ntok)), lambda N: True)
TEXT_MUTANTS["key and value slabs swapped"] = (
    lambda fs, xf, ntok: (lambda a, k, v: (a, v, k))(*text_state(fs, xf, ntok)), lambda N: True)


# ------------------------------------------------------------------------------------------------------------------------
# tolerances
# ------------------------------------------------------------------------------------------------------------------------
# MEASURED[stage][width][precision]: the error of the oracle under frame_rounding(precision) against the plain oracle in the
# stage's metric, worst over the stage's cases (tests/test_frame_probe_host.py re-measures it).  No figure comes from a kernel.
# The stem cache and the text cache are computed in the bf16x3 arithmetic whatever the mode: one figure for all four.
MEASURED = {
    "stem": {
        "tiny": {3: 1.5e-05, 1: 8.2e-03},
        "small": {3: 1.4e-05, 4: 1.4e-05, 2: 6.6e-04, 1: 6.0e-03},
        "big": {3: 1.3e-05, 4: 1.3e-05, 2: 6.8e-04, 1: 5.2e-03},
        "tools": {3: 1.3e-05, 4: 1.3e-05, 2: 7.0e-04, 1: 5.5e-03},
    },
    "stem_cache": {
        "small": {3: 1.3e-05, 4: 1.3e-05, 2: 1.3e-05, 1: 1.3e-05},
        "big": {3: 1.0e-05, 4: 1.0e-05, 2: 1.0e-05, 1: 1.0e-05},
        "tools": {3: 1.3e-05, 4: 1.3e-05, 2: 1.3e-05, 1: 1.3e-05},
    },
    "embed_down": {
        "small": {3: 7.0e-05, 4: 7.0e-05, 2: 5.6e-03, 1: 4.4e-02},
        "big": {3: 6.2e-05, 4: 6.2e-05, 2: 4.9e-03, 1: 4.4e-02},
        "tools": {3: 6.9e-05, 4: 6.9e-05, 2: 6.3e-03, 1: 5.5e-02},
    },
    "block0": {
        "small": {3: 7.3e-05, 4: 7.3e-05, 2: 6.0e-03, 1: 4.4e-02},
        "big": {3: 6.2e-05, 4: 6.2e-05, 2: 5.0e-03, 1: 4.5e-02},
        "tools": {3: 6.6e-05, 4: 6.6e-05, 2: 6.2e-03, 1: 5.3e-02},
    },
    "up_skip": {
        "small": {3: 7.7e-05, 4: 7.7e-05, 2: 5.5e-03, 1: 4.9e-02},
        "big": {3: 6.4e-05, 4: 6.4e-05, 2: 4.8e-03, 1: 3.9e-02},
        "tools": {3: 6.4e-05, 4: 6.4e-05, 2: 5.4e-03, 1: 4.3e-02},
    },
    "head": {
        "small": {3: 2.5e-06, 4: 2.5e-06, 2: 2.3e-04, 1: 1.8e-03},
        "big": {3: 2.6e-06, 4: 2.6e-06, 2: 2.0e-04, 1: 1.7e-03},
        "tools": {3: 2.6e-06, 4: 2.6e-06, 2: 2.2e-04, 1: 1.8e-03},
    },
    # two correct stems seen through slot 0 of layer 0 (stem_pair): the gate between a forward with and without a stem cache
    "stem_pair": {
        "small": {3: 1.1e-05, 4: 1.1e-05, 2: 7.2e-04, 1: 5.8e-03},
        "big": {3: 8.9e-06, 4: 8.9e-06, 2: 6.4e-04, 1: 4.7e-03},
        "tools": {3: 9.7e-06, 4: 9.7e-06, 2: 6.3e-04, 1: 4.3e-03},
    },
    "text_cache": {
        "small": {3: 8.5e-06, 4: 8.5e-06, 2: 8.5e-06, 1: 8.5e-06},
        "big": {3: 7.6e-06, 4: 7.6e-06, 2: 7.6e-06, 1: 7.6e-06},
        "tools": {3: 8.2e-06, 4: 8.2e-06, 2: 8.2e-06, 1: 8.2e-06},
    },
}

# The claim is made per (mutant, case, precision): every one is at least POWER tolerances away, except the entries below, each
# recorded with the ratio (distance / tolerance) it measures and asserted by the host test to be below the bar and where it was
# recorded, so that neither list can grow stale or hide a case: {(stage, width): {mutant: (reason, {case: ratio})}}, the case being
# B for the stem and (B, T, lengths) for the frame.
_T1 = ("one timestep moves emb and the (scale | shift) rows by 5e-2 ... 1.2e-1 of a row, under 4 bf16 tolerances of the plain stem "
       "(4 x 5.2e-3 ... 8.2e-3: mix, the post_mlp rows and e1 are bf16 rows); the stem-cache table, fp32-grade in every mode, "
       "sees it at 6000 tolerances and fp16 at 19 or more")
_LEN = ("one coarse key more among n moves the Performer's key-value sum, which every valid frame shares, by 1 / (n + 1): 0.9 of "
        "the branch at n = 1, 0.24 at n = 15, 0.07 at n = 97, against a bf16 tolerance of the dual block it is read through of "
        "4 x 4.4e-2 ... 5.5e-2; modes 3 / 4 see every case at 235 or more")
_LEN2 = ("an unhalved length adds 1 ... 16 keys (at T = 196 one, as ceil does): 0.56 ... 1.0 of the branch and 0.07 at n = 97, "
         "against the same bf16 tolerance")
_C6, _C14, _C34, _C66, _C196 = (3, 6, (6, 5, 1)), (3, 14, (14, 13, 3)), (5, 34, (34, 33, 17, 1, 0)), (2, 66, (66, 31)), (2, 196, (196, 195))
BF16_OUT_OF_REACH = {
    ("stem", "tiny"): {"timestep + 1": (_T1, {1: 1.5, 3: 1.9, 33: 3.1, 130: 3.6}), "timestep - 1": (_T1, {1: 1.5, 3: 1.7, 33: 2.9, 130: 3.2})},
    ("stem", "small"): {"timestep + 1": (_T1, {1: 3.8, 3: 3.7, 33: 3.9}), "timestep - 1": (_T1, {1: 3.6, 3: 3.7, 33: 4.0})},
    ("stem", "big"): {"timestep - 1": (_T1, {1: 3.9})},
    ("stem", "tools"): {"timestep + 1": (_T1, {1: 2.7}), "timestep - 1": (_T1, {1: 2.4})},
    ("embed_down", "small"): {"coarse length ceil(len / 2)": (_LEN, {_C34: 1.6, _C66: 1.4, _C196: 0.37}),
                              "coarse length len": (_LEN2, {_C196: 0.37})},
    ("embed_down", "big"): {"coarse length ceil(len / 2)": (_LEN, {_C6: 3.2, _C34: 1.8, _C66: 1.7}), "coarse length len": (_LEN2, {_C6: 3.2})},
    ("embed_down", "tools"): {"coarse length ceil(len / 2)": (_LEN, {_C6: 3.2, _C14: 3.6, _C34: 2.2, _C66: 1.1, _C196: 0.32}),
                              "coarse length len": (_LEN2, {_C6: 3.2, _C66: 2.6, _C196: 0.32})},
}
# The one exception in a mode other than bf16.  The sample of 195 frames has 97 coarse keys; key 98 moves the branch by 6.6e-2 ...
# 7.1e-2, and no frame by more: the Performer is linear attention (num = phi(q) . sum_k phi(k) v^T, one sum for all frames) and
# the LayerNorm behind num / den removes the per-frame denominator, so the frame that becomes valid and the frames next to it see
# the same 1 / 98 as every other.  That is 2.8 ... 2.9 fp16 tolerances (4 x 5.6e-3 ... 6.3e-3): a device with this fault still
# misses the gate of 1 here, with a margin of 2.8 where the project asks for 4.  The same floor is held at 9.7 or more fp16
# tolerances by the samples of 31, 33, 13 and 5 frames, and the halved length is one elementwise operation whatever T is.
_LEN97 = ("one key more among 97 moves the branch by 1 / 98 in every frame alike (linear attention: one key-value sum; the "
          "LayerNorm removes the per-frame denominator): under 4 fp16 tolerances, while n <= 15 holds the same floor at 9.7 or more")
FP16_EXCEPTION_CASE = _C196
FP16_BELOW_THE_BAR = {
    ("embed_down", "small"): {"coarse length ceil(len / 2)": (_LEN97, {_C196: 2.9}), "coarse length len": (_LEN97, {_C196: 2.9})},
    ("embed_down", "tools"): {"coarse length ceil(len / 2)": (_LEN97, {_C196: 2.8}), "coarse length len": (_LEN97, {_C196: 2.8})},
}
# the mutants that no mode may be excused from (the pairing, tap-swap, slot, slab, row-roll and skip mutants)
NEVER_OUT_OF_REACH = (
    "sample rows rolled by one", "slot j delivered in slot j + 1", "scale and shift halves swapped",
    "slots of layer i swapped with layer i + 1", "frame pairs (2i + 1, 2i + 2)", "taps of downsample.weight swapped",
    "slab of layer j delivered for layer j + 1", "key and value slabs swapped", "rows rolled by one") + tuple(UP_MUTANTS)


# The share of the fp32-grade figure that the hook measures with exact sinusoid frequencies (frame_rounding(3, ulp=False)); the
# rest of MEASURED["stem" / "stem_cache"][...][3 | 4] is the allowance for the device's expf, which nothing here measures.
SINUSOID_ULP_SHARE = {("stem", "tiny"): 0.95, ("stem", "small"): 0.79, ("stem", "big"): 0.75, ("stem", "tools"): 0.83,
                      ("stem_cache", "small"): 1.0, ("stem_cache", "big"): 1.06, ("stem_cache", "tools"): 0.98}


def tol(stage, width, precision):
    return MARGIN * MEASURED[stage][width][precision]
