"""Host: the power proof of tests/test_frame_selective_gpu.py, from the oracle alone (no GPU).

The pieces restated in tests/frame_probe.py equal the oracle bit for bit with every switch off; frame_probe.MEASURED is what the
oracle under frame_rounding gives; every mutant is at least POWER x MARGIN x MEASURED away from the oracle in its stage's metric,
at every precision the stage runs and in every case that exercises it, except the (stage, width, mutant, case) entries of
frame_probe.BF16_OUT_OF_REACH at bf16 and of frame_probe.FP16_BELOW_THE_BAR at fp16 (one sample of 97 coarse frames) -- each of
which is asserted to be below the bar, at the ratio recorded for it."""
import pytest
import torch

import frame_probe as FP

R = FP.R
AP = FP.AP


# ------------------------------------------------------------------------------------------------------------------------
# the restated pieces are the oracle's
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["tools", "tiny"])
def test_the_restated_stem_is_the_oracles_bit_for_bit(width):
    fs = FP.frame_state(width)
    ts, xp = FP.stem_inputs(width, 3)
    with torch.no_grad():
        emb, sc = FP.stem(fs, ts, xp)
        ref = R.fused_embedding(fs["sd"], ts, xp, fs["D"], fs["eph"])
        assert torch.equal(FP.sinusoid(ts, fs["D"]), R.sinusoid(ts, fs["D"]))
        assert torch.equal(emb, ref)
        for j, (pre, name) in enumerate(FP.slot_prefixes(fs["L"])):
            # the (scale | shift) rows as R.stylization forms them from emb (stylization.py:22-27)
            w, b = fs["eph"][name]
            want = R._lin(torch.nn.functional.silu(torch.nn.functional.linear(ref, w, b)), fs["sd"], pre + ".emb_layers.1")
            assert torch.equal(sc[j], want), name


@pytest.mark.parametrize("width", ["small", "tools"])
def test_the_restated_frame_is_the_oracles_bit_for_bit(width):
    """embed, down, the halved lengths, up + skip, the head and the dual block with given (scale | shift) rows against
    R.denoiser_forward's trace, with every switch off."""
    fs = FP.frame_state(width)
    case = FP.CASES[2]
    inp = FP.frame_inputs(width, case)
    B, T = inp["B"], inp["T"]
    N = 5
    xf = FP.pkg("synth").uniform_pm1((B, N, fs["Dt"]), "frame.host.xf", 1)
    cfg = dict(latent_dim=fs["D"], num_heads=fs["H"], num_layers=fs["L"], moe_num_experts=fs["E"])
    trace = {}
    with torch.no_grad():
        out = R.denoiser_forward(fs["sd"], cfg, inp["x"], inp["ts"], inp["length"], inp["xp"], xf, fs["eph"], fs["proj"], None, trace)
        assert torch.equal(inp["emb"], trace["fused_emb"]) and torch.equal(inp["h"], trace["h_embed"])
        assert torch.equal(inp["h_low"], trace["h_low"])
        assert torch.equal(inp["lo"], trace["decoder_blocks_low.0.module.dual_self_attn"])
        last_low = trace[f"decoder_blocks_low.{fs['L'] - 1}.module.sd_cross_attn"]
        hc = FP.up_skip(fs, last_low, inp["h"])
        assert torch.equal(hc, trace["h_combined"])
        assert torch.equal(FP.read_high(fs, inp, hc), trace["decoder_blocks_high.0.module.dual_self_attn"])
        assert torch.equal(FP.head(fs, trace[f"decoder_blocks_high.{fs['L'] - 1}.module.sd_cross_attn"]), out)
    assert FP._CUR.r is FP._ID and AP._LIN is R._lin and AP._STATE is R.linear_cross_text_state  # every swap was undone


def test_the_restated_text_state_is_the_oracles_bit_for_bit():
    fs = FP.frame_state("tools")
    xf, _ = FP.text_inputs("tools", 6)
    at, k, v = FP.text_state(fs, xf, (6, 6, 6))
    with torch.no_grad():
        for li, pre in enumerate(FP.layer_prefixes(fs["L"])):
            assert torch.equal(at[li], R.linear_cross_text_state(xf, fs["sd"], pre + ".cross_attn.base_ca", fs["H"]))
            assert torch.equal(k[li], R._lin(xf, fs["sd"], pre + ".sd_cross_attn.key"))
            assert torch.equal(v[li], R._lin(xf, fs["sd"], pre + ".sd_cross_attn.value"))


# ------------------------------------------------------------------------------------------------------------------------
# the survey: rounding error and mutant distances per (stage, width)
# ------------------------------------------------------------------------------------------------------------------------
_SURVEY, _NO_ULP = {}, {}


def _stem_survey(width):
    fs, fs64 = FP.frame_state(width), FP.as64(FP.frame_state(width))
    precisions = FP.PRECISIONS[width]
    worst, dist, plain = {p: 0.0 for p in precisions}, {}, 0.0
    for B in FP.STEM_BATCHES:
        ts, xp = FP.stem_inputs(width, B)
        ref = FP.stem(fs64, ts, xp)
        for p in precisions:
            with FP.frame_rounding(p, acts16=width != "tiny"):
                worst[p] = max(worst[p], FP.stem_metric(FP.stem(fs, ts, xp), ref))
        with FP.frame_rounding(3, ulp=False):
            plain = max(plain, FP.stem_metric(FP.stem(fs, ts, xp), ref))
        for name, (fn, applies) in FP.STEM_MUTANTS.items():
            if applies(fs, B):
                dist[name, B] = FP.stem_metric(fn(fs64, ts, xp), ref)
    _NO_ULP["stem", width] = plain
    return worst, dist


def _cache_survey(width):
    fs, fs64 = FP.frame_state(width), FP.as64(FP.frame_state(width))
    steps = FP.STEM_CACHE_STEPS[width]
    _, xp = FP.stem_inputs(width, FP.STEM_CACHE_BATCH)
    ref = FP.stem_cache(fs64, steps, xp)
    with FP.frame_rounding(3):
        w = FP.stem_metric(FP.stem_cache(fs, steps, xp), ref)
    with FP.frame_rounding(3, ulp=False):
        _NO_ULP["stem_cache", width] = FP.stem_metric(FP.stem_cache(fs, steps, xp), ref)
    dist = {(name, steps): FP.stem_metric(fn(fs64, steps, xp), ref) for name, fn in FP.CACHE_MUTANTS.items()
            if not (name == "text_proj skipped" and fs["Dt"] == fs["D"])}
    return {p: w for p in FP.PRECISIONS[width]}, dist


def _frame_survey(width):
    """embed_down, block0, up_skip and head in one pass over the cases."""
    fs, fs64 = FP.frame_state(width), FP.as64(FP.frame_state(width))
    precisions = FP.PRECISIONS[width]
    worst = {s: {p: 0.0 for p in precisions} for s in ("embed_down", "block0", "up_skip", "head")}
    dist = {s: {} for s in worst}
    with torch.no_grad():
        for case in FP.cases_of(width):
            inp = FP.frame_inputs(width, case)
            low = lambda t: FP.branch_metric(fs, t, inp["lo"], inp["base_lo"], inp["len_low"])[2]
            high = lambda t: FP.branch_metric(fs, t, inp["hi"], inp["base_hi"], inp["length"])[2]
            head_ref = FP.head(fs64, inp["hi"])
            for p in precisions:
                with FP.frame_rounding(p):
                    worst["embed_down"][p] = max(worst["embed_down"][p], low(FP.read_low(fs, inp, FP.down(fs, FP.embed(fs, inp["x"])))))
                    worst["up_skip"][p] = max(worst["up_skip"][p], high(FP.read_high(fs, inp, FP.up_skip(fs, inp["x_low"], inp["h"]))))
                    worst["head"][p] = max(worst["head"][p], FP.per_sample_rel(FP.head(fs, inp["hi"]), head_ref))
                    _, sc = FP.stem(fs, inp["ts"], inp["xp"])
                    worst["block0"][p] = max(worst["block0"][p], low(FP.read_low(fs, inp, FP.down(fs, FP.embed(fs, inp["x"])), sc=sc)))
            for name, (fn, applies) in FP.EMBED_MUTANTS.items():
                if applies(case):
                    dist["embed_down"][name, case] = low(fn(fs, inp))
            for name, fn in FP.UP_MUTANTS.items():
                dist["up_skip"][name, case] = high(fn(fs, inp))
            for name, fn in FP.HEAD_MUTANTS.items():
                dist["head"][name, case] = FP.per_sample_rel(fn(fs64, inp["hi"]), head_ref)
    return worst, dist


def _text_survey(width):
    fs, fs64 = FP.frame_state(width), FP.as64(FP.frame_state(width))
    w, dist = 0.0, {}
    for N in FP.TEXT_N:
        xf, ntok = FP.text_inputs(width, N)
        ref = FP.text_state(fs64, xf, ntok)
        with AP.rounding(3):
            w = max(w, FP.text_metric(FP.text_state(fs, xf, ntok), ref, ntok))
        for name, (fn, applies) in FP.TEXT_MUTANTS.items():
            if applies(N):
                dist[name, N] = FP.text_metric(fn(fs64, xf, ntok), ref, ntok)
    return {p: w for p in FP.PRECISIONS[width]}, dist


def survey(stage, width):
    """(worst rounding-hook error per precision, {(mutant, case): distance}) of a stage at a width, in the stage's metric."""
    if stage in ("embed_down", "block0", "up_skip", "head"):
        if ("frame", width) not in _SURVEY:
            _SURVEY["frame", width] = _frame_survey(width)
        worst, dist = _SURVEY["frame", width]
        return worst[stage], dist[stage]
    if (stage, width) not in _SURVEY:
        _SURVEY[stage, width] = {"stem": _stem_survey, "stem_cache": _cache_survey, "text_cache": _text_survey}[stage](width)
    return _SURVEY[stage, width]


STAGES = [(s, w) for s in ("stem", "stem_cache", "embed_down", "block0", "up_skip", "head", "text_cache")
          for w in (("tiny",) if s == "stem" else ()) + FP.FRAME_WIDTHS]


@pytest.mark.parametrize("stage,width", STAGES, ids=lambda v: str(v))
def test_tolerances_are_the_measured_rounding_error(stage, width):
    """frame_probe.MEASURED is not below what the oracle under the rounding hook gives here (one-sided, with 15 % for what thread
    counts and BLAS kernels do to an inf-norm of rounding noise), for exactly the precisions the stage runs."""
    worst, _ = survey(stage, width)
    rec = FP.MEASURED.get(stage, {}).get(width, {})
    print(stage, width, "measured", {p: f"{v:.2e}" for p, v in worst.items()}, "recorded", rec, "tolerance",
          {p: f"{FP.MARGIN * v:.1e}" for p, v in rec.items()})
    assert set(worst) == set(rec)
    for p, v in worst.items():
        assert v < rec[p] * 1.15, (p, v)
        assert rec[p] < max(v * 2.0, 1e-6), (p, v)  # nor a multiple of it


def test_the_sinusoid_allowance_is_a_stated_share_of_the_fp32_grade_figures():
    """The stem and stem-cache figures of modes 3 / 4 include frequencies one fp32 ulp off, an allowance for the device's own
    expf that no 16-bit store of the code accounts for.  Without it the hook measures the SINUSOID_ULP_SHARE recorded in
    frame_probe of the figure with it: 0.75 ... 0.95 of the plain stem's (a quarter of that gate at most is allowance) and all
    of the stem cache's (none of it is).  Printed, and asserted, so that the share can be read."""
    for (stage, width), share in FP.SINUSOID_ULP_SHARE.items():
        worst, _ = survey(stage, width)
        got = _NO_ULP[stage, width] / worst[3]
        print(f"{stage} {width}: {_NO_ULP[stage, width]:.2e} without the allowance, {worst[3]:.2e} with it: {got:.2f} of the figure")
        assert share / 1.25 < got < share * 1.25, (stage, width, got)


# mode-2 figures of the plain stem under the arithmetic it had before the fix (single pass on the bf16 hi plane), fwd_tools_shape
SINGLE_PASS = {"measured": 5.3e-3, "timestep ratio below": FP.POWER}


def test_the_single_pass_chain_was_too_coarse_for_the_fp16_mode():
    """The finding behind `c3` in stem_embeddings, from the oracle alone: with the time and text chains as one pass on the bf16
    hi plane, an fp16 run's stem is 5.3e-3 off where its other rows hold 7e-4, and timestep +- 1 is then under 4 tolerances."""
    fs, fs64 = FP.frame_state("tools"), FP.as64(FP.frame_state("tools"))
    worst, near = 0.0, 1e30
    for B in FP.STEM_BATCHES:
        ts, xp = FP.stem_inputs("tools", B)
        ref = FP.stem(fs64, ts, xp)
        with FP.frame_rounding(2, single_pass_chain=True):
            worst = max(worst, FP.stem_metric(FP.stem(fs, ts, xp), ref))
        near = min(near, *(FP.stem_metric(FP.STEM_MUTANTS[n][0](fs64, ts, xp), ref) for n in ("timestep + 1", "timestep - 1")))
    print(f"plain stem, tools, mode 2, single-pass chains: {worst:.2e} (now {FP.MEASURED['stem']['tools'][2]:.1e}); timestep +- 1 at "
          f"{near / (FP.MARGIN * worst):.1f} such tolerances")
    assert SINGLE_PASS["measured"] / 1.15 < worst < SINGLE_PASS["measured"] * 1.15
    assert worst > 5 * FP.MEASURED["stem"]["tools"][2]
    assert near / (FP.MARGIN * worst) < SINGLE_PASS["timestep ratio below"]


def _listed(stage, width, p):
    return {1: FP.BF16_OUT_OF_REACH, 2: FP.FP16_BELOW_THE_BAR}.get(p, {}).get((stage, width), {})


@pytest.mark.parametrize("stage,width", [sw for sw in STAGES if sw[0] != "block0"], ids=lambda v: str(v))
def test_every_mutant_is_four_tolerances_away(stage, width):
    """Per (mutant, case, precision): at least POWER tolerances away, or listed for exactly that case and precision, below the
    bar, at the ratio recorded for it."""
    _, dist = survey(stage, width)
    bad, stale, low, seen = [], [], {}, set()
    for (name, case), d in dist.items():
        for p in FP.PRECISIONS[width]:
            ratio = d / FP.tol(stage, width, p)
            low[name, p] = min(low.get((name, p), 1e30), ratio)
            rec = _listed(stage, width, p).get(name, (None, {}))[1].get(case)
            if rec is None:
                if not ratio >= FP.POWER:
                    bad.append((name, case, p, round(ratio, 2)))
            else:
                seen.add((name, case, p))
                if not (ratio < FP.POWER and rec / 1.25 < ratio < rec * 1.25):
                    stale.append((name, case, p, round(ratio, 2), rec))
    for (name, p), r in sorted(low.items()):
        print(f"{stage} {width}: {name!r} precision {p}: >= {r:.1f} tolerances in every case")
    assert not bad, bad
    assert not stale, stale
    for p in (1, 2):
        for name, (_, cases) in _listed(stage, width, p).items():
            assert all((name, case, p) in seen for case in cases), (name, p, "lists a case that is not measured")


def test_the_out_of_reach_lists_hold_only_what_they_may():
    """Modes 3 and 4 have no list.  Mode 1: neither the pairing, tap-swap, slot, slab, row-roll and skip mutants nor anything of
    the stem-cache table.  Mode 2, where the issue admits nothing: the two coarse-length mutants at the one case whose changed
    sample has 97 coarse frames, and nothing else -- every other case that changes a coarse length claims them in mode 2
    (test_every_mutant_is_four_tolerances_away: what is not listed for a case is asserted there)."""
    for (stage, width), names in FP.BF16_OUT_OF_REACH.items():
        assert stage != "stem_cache", "the stem-cache table is fp32-grade in every mode"
        for name, (reason, cases) in names.items():
            assert name not in FP.NEVER_OUT_OF_REACH, (stage, width, name)
            assert len(reason) > 40 and cases
    for (stage, width), names in FP.FP16_BELOW_THE_BAR.items():
        assert stage == "embed_down"
        for name, (reason, cases) in names.items():
            assert name in ("coarse length ceil(len / 2)", "coarse length len") and len(reason) > 40
            assert set(cases) == {FP.FP16_EXCEPTION_CASE}, (stage, width, name)
            others = [c for c in FP.cases_of(width) if c != FP.FP16_EXCEPTION_CASE and FP.EMBED_MUTANTS[name][1](c)]
            assert len(others) >= 4 and (2, 66, (66, 31)) in others  # claimed in mode 2 at T = 6, 14, 34 and 66


# (width, timestep shift) -> distance in the block0 metric, recorded from this test's own print
GATHER_OFF_BY_ONE = {("small", 1): 1.3e-2, ("small", -1): 1.5e-2, ("big", 1): 1.1e-2, ("big", -1): 9.6e-3, ("tools", 1): 9.9e-3,
                     ("tools", -1): 9.8e-3}


@pytest.mark.parametrize("width", FP.FRAME_WIDTHS)
def test_a_gather_one_row_off_is_seen_between_the_two_forwards_in_every_mode(width):
    """What test_forward_with_and_without_the_stem_cache can claim.  The C ABI hands out no tensor between gated_mix_gather and
    the first block, so a stem cache read one row off (timestep +- 1) is seen through slot 0 of layer 0.  Against the oracle
    (block0) that is 37 or more tolerances in modes 3 and 4 and under one in modes 2 and 1.  Between the two forwards the dual
    block's own rounding cancels and what is left is how far two correct stems are apart (frame_probe.stem_pair, from the oracle:
    the plain stem and the cached one run the same bf16x3 chains in another fp32 summation order, and the 16-bit rows behind
    them -- mix, the post_mlp hidden rows, emb, e1 -- each turn that into flips of one 16-bit ulp, so that at e1 the two are a
    rounding of that format apart).  There the fault is 200 or more tolerances away in modes 3 and 4 and 3.9 ... 5 in mode 2:
    at least twice the gate, so a device within its gate of the truth cannot carry it unseen.  In mode 1 it is 0.5 ... 0.6
    of the gate between the forwards too: nothing the ABI hands out shows a wrong bf16 gather, asserted here so that the claim
    stays what it is.  The 16-bit modes run the same kernel with the same index arithmetic and differ in the store alone; the
    table itself is held at 6000 tolerances in every mode (stem_cache)."""
    fs = FP.frame_state(width)
    inp = FP.frame_inputs(width, FP.PAIR_CASE, ts=FP.pair_timesteps(width))
    rec = FP.MEASURED["stem_pair"][width]
    with torch.no_grad():
        pair = {p: FP.stem_pair(fs, inp, p) for p in FP.PRECISIONS[width]}
        print(f"stem_pair {width}: measured", {p: f"{v:.2e}" for p, v in pair.items()}, "recorded", rec)
        for p, v in pair.items():
            assert v < rec[p] * 1.5 and rec[p] < max(v * 4.0, 1e-6), (p, v)  # which values flip is chance: a noisier figure
        for shift in (1, -1):
            _, sc = FP.stem(fs, inp["ts"] + shift, inp["xp"])
            d = FP.branch_metric(fs, FP.read_low(fs, inp, inp["h_low"], sc=sc), inp["lo"], inp["base_lo"], inp["len_low"])[2]
            ratios = {p: d / FP.tol("block0", width, p) for p in FP.PRECISIONS[width]}
            between = {p: d / FP.tol("stem_pair", width, p) for p in FP.PRECISIONS[width]}
            print(f"block0 {width}: timestep {shift:+d} moves slot 0 of layer 0 by {d:.2e}:", {p: f"{r:.1f}" for p, r in ratios.items()},
                  "tolerances against the oracle,", {p: f"{r:.1f}" for p, r in between.items()}, "between the two forwards")
            assert GATHER_OFF_BY_ONE[width, shift] / 1.5 < d < GATHER_OFF_BY_ONE[width, shift] * 1.5
            assert ratios[3] >= FP.POWER and ratios[4] >= FP.POWER and ratios[2] < FP.POWER and ratios[1] < FP.POWER
            assert between[3] >= FP.POWER and between[4] >= FP.POWER and between[2] >= 2.0 and between[1] < 1.0, between
