"""GPU: a module's forward must not depend on its history -- on the precisions it ran at before (``precision`` is a plain attribute
that callers switch on a live module) or on the packs it built before its weights, ephemeral Linears or Performer projections were
replaced.  Every result is compared bit for bit with a module built fresh in the state under test, on the 1-layer goldens of both
widths (D = 512 and D = 1024, whose packs carry different weight streams)."""
import pytest
import torch

from conftest import build_module, golden_state, load_golden, pkg, rel_inf

pytestmark = pytest.mark.gpu

CASES = ["fwd_small_dims", "fwd_big_dims"]  # D = 512, B = 2, T = 16 | D = 1024, B = 2, T = 8
PRECS = (1, 2, 3, 4, 5)
TOL_FP32 = 1e-3  # the gate of test_forward_gpu.py::test_forward_matches_reference_fp32_grade

_GOLD = {}   # case -> (golden tensors, meta, forward args, forward kwargs)
_FRESH = {}  # (case, precision) -> module built at that precision and never switched
_OUT = {}    # (case, precision) -> that module's forward on the golden inputs, or the library's refusal


@pytest.fixture(scope="module", autouse=True)
def _release_modules():
    yield
    _FRESH.clear(), _OUT.clear(), _GOLD.clear()


def _case(case):
    if case not in _GOLD:
        g, meta = load_golden(case)
        args = (g["x"].cuda(), g["timesteps"].cuda(), g["length"].cuda())
        _GOLD[case] = (g, meta, args, dict(xf_proj=g["xf_proj"].cuda(), xf_out=g["xf_out"].cuda()))
    return _GOLD[case]


def _fresh(case, precision):
    if (case, precision) not in _FRESH:
        _FRESH[case, precision] = build_module(_case(case)[1], precision=precision)[0]
    return _FRESH[case, precision]


def _fresh_out(case, precision):
    """Forward of the fresh module (memoised).  A precision the library refuses at this shape skips the test with its reason;
    only the fp8 mode may be refused (its expert GEMMs need K % 128 == 0)."""
    L = pkg("_lib")
    if (case, precision) not in _OUT:
        _, _, args, kw = _case(case)
        try:
            _OUT[case, precision] = _fresh(case, precision)(*args, **kw)
        except L.MdmError as e:
            if precision != L.PREC_FP8:
                raise
            _OUT[case, precision] = e
    y = _OUT[case, precision]
    if isinstance(y, L.MdmError):
        pytest.skip(f"precision {precision} refused at {case}: {y}")
    return y


def _differ(a, b):
    return f"max |diff| {float((a - b).abs().max()):.3e}"


@pytest.mark.parametrize("p,q", [(p, q) for p in PRECS for q in PRECS if p != q])
@pytest.mark.parametrize("case", CASES)
def test_precision_history_does_not_change_the_forward(case, p, q):
    """Run at p, set ``precision = q`` without invalidate(), run again: the result is the fresh q-module's, bit for bit (a pack
    built for p must never serve q: the two can read the same planes but not the same weight streams)."""
    g, meta, args, kw = _case(case)
    want_p, want_q = _fresh_out(case, p), _fresh_out(case, q)
    m, _ = build_module(meta, precision=p)
    y_p = m(*args, **kw)
    assert torch.equal(y_p, want_p), _differ(y_p, want_p)
    m.precision = q
    y_q = m(*args, **kw)
    assert torch.equal(y_q, want_q), (f"{case}: precision {p} -> {q}", _differ(y_q, want_q))
    if q == 3:
        err = rel_inf(y_q.cpu(), g["output"])
        print(f"{case}: precision {p} -> 3, rel err vs the reference golden {err:.2e}")
        assert err < TOL_FP32, err


@pytest.mark.parametrize("case", CASES)
def test_switching_back_and_forth(case):
    """1 -> 3 -> 1 -> 3 on one module: every result is the fresh module's for its precision (a pack that is rebuilt, reused or
    overwritten in the wrong order shows up as a mismatch on the way back)."""
    _, meta, args, kw = _case(case)
    want = {q: _fresh_out(case, q) for q in (1, 3)}
    assert not torch.equal(want[1], want[3])  # the two modes really compute different things
    m, _ = build_module(meta, precision=1)
    for i, q in enumerate((1, 3, 1, 3)):
        m.precision = q
        y = m(*args, **kw)
        assert torch.equal(y, want[q]), (f"{case}: run {i} at precision {q}", _differ(y, want[q]))


def _struct_packed(pm):
    """Every MdmPacked of the model struct, under its kernel_layout() name."""
    L = pkg("_lib")
    out = {n: getattr(pm.model, n) for n in L._MODEL_PACKED + ["style_eph", "style_emb"] if n in pm.W}
    for li in range(2 * pm.cfg["num_layers"]):
        k, l = f"L{li}.", pm.layers[li]
        for which, perf in (("local", l.local), ("global", l.global_)):
            for nm in ("qkv", "feat", "proj0", "proj3"):
                out[f"{k}{which}.{nm}"] = getattr(perf, nm)
            out[f"{k}{which}.style.out"] = perf.style.out
        for nm in ("skip", "ca_q", "ca_k", "ca_v", "w1", "w2", "sd_q", "sd_k", "sd_v", "sd_out", "sd_f1", "sd_f2"):
            out[k + nm] = getattr(l, nm)
        out[k + "ca_style.out"], out[k + "ffn_style.out"] = l.ca_style.out, l.ffn_style.out
    return out


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("case", CASES)
def test_packed_streams_match_their_consumer(case, precision):
    """Structural audit of pack() (no kernel launch beyond packing): MdmPacked.ws carries a (hi, lo) pair stream of an expert matrix
    in the fp32-grade mode only, sized mdm_gemm_stream3x_elems(2E, N, K) -- what moe_block hands gemm_stream3x; a 16-bit fragment
    stream (mdm_gemm_stream1_elems(N, K), in the format of the matrix's planes) of a plain Linear in the 16-bit modes only -- what
    linear() hands gemm_stream1 -- and never of an expert matrix, which no 16-bit launch reads through MdmPacked.ws."""
    L = pkg("_lib")
    lib = L.lib()
    ops = pkg("ops")
    pm = _fresh(case, precision).pack()
    plan = pkg("packing").stream_plan(pm.cfg, precision)
    assert pm.plan == plan
    # pm.streams: the packed entries of the plan by key; the MdmPacked.ws streams by the name of their matrix
    pairs = {s.sources[0]: pm.streams[s.key] for s in plan if s.kind == "expert3" and s.key in pm.streams}
    frag = {s.sources[0]: pm.streams[s.key] for s in plan if s.kind == "frag" and s.key in pm.streams}
    D, F, E2 = pm.cfg["latent_dim"], pm.cfg["ff_size"], 2 * pm.cfg["moe_num_experts"]
    experts = {"w1": (F, D), "w2": (D, F)}  # [2E * N, K] stacked
    sixteen_bit = precision in (L.PREC_BF16, L.PREC_F16, L.PREC_FP8)
    assert not [n for n in frag if n.rsplit(".", 1)[1] in experts], "expert matrices must not carry a 16-bit stream"
    assert sixteen_bit or not frag, "fragment streams exist for the 16-bit modes only"
    if D == 1024 and sixteen_bit:
        assert frag, "the D = 1024 model streams its per-layer Linears in the 16-bit modes"
    for name, ws in frag.items():
        N, K = pm.W[name].N, pm.W[name].K
        h16 = torch.float16 if pm.W[name].fmt == "f16" else torch.bfloat16  # (the text-side Linears keep bf16 planes in every mode)
        assert ws.dtype == h16 and ws.numel() == lib.mdm_gemm_stream1_elems(N, K) > 0, (name, ws.dtype, ws.numel())
    assert precision == L.PREC_X3 or not pairs, "pair streams exist for the fp32-grade mode only"
    for li in range(2 * pm.cfg["num_layers"]):
        for nm, (N, K) in experts.items():
            name = f"L{li}.{nm}"
            ws = getattr(pm.layers[li], nm).ws or 0
            n = lib.mdm_gemm_stream3x_elems(E2, N, K) if precision == L.PREC_X3 else 0
            if n > 0:
                assert ws == pairs[name].data_ptr() and pairs[name].numel() == n, (name, pairs[name].numel(), n)
            else:
                assert ws == 0 and name not in pairs, name
    if precision == L.PREC_X3:
        assert pairs, "the fp32-grade model streams its expert matrices (w1: K = D in {512, 1024}, N = F % 512 == 0)"
    # every stream is the one its MdmPacked points at, and every non-null MdmPacked.ws is one of these streams
    packed = _struct_packed(pm)
    assert not set(frag) & set(pairs) and set(frag) | set(pairs) <= set(packed)
    for name, p in packed.items():
        ws = frag.get(name, pairs.get(name))
        assert (p.ws or 0) == (ws.data_ptr() if ws is not None else 0), name
    # the same for all six stream fields: what is packed is what the plan asks for and the library takes, every packed stream's
    # pointer is in its slot, and every other stream field of the model is null
    assert set(pm.streams) == {s.key for s in plan if ops.stream_elems(s.kind, *s.shape) > 0}
    want = {s.slot: pm.streams[s.key].data_ptr() for s in plan if s.key in pm.streams}
    assert len(want) == len(pm.streams) == len({t.data_ptr() for t in pm.streams.values()})
    for s in plan:
        if s.key in pm.streams:
            assert getattr(pm.slot_struct(s.slot), s.slot.field) == want[s.slot], s
            assert pm.streams[s.key].dtype == (torch.float16 if s.h16 == "f16" else torch.bfloat16), s
    Slot = pkg("packing").Slot
    have = {Slot("packed", name, "ws"): p.ws for name, p in packed.items()}
    for li in range(2 * pm.cfg["num_layers"]):
        k, l = f"L{li}.", pm.layers[li]
        have[Slot("layer", k, "wstream")], have[Slot("layer", k, "sd_ffn_ws")] = l.wstream, l.sd_ffn_ws
        assert l.wstream_gs == (2 * D * F if l.wstream else 0)
        styles = [(k + "ca_style.", l.ca_style), (k + "ffn_style.", l.ffn_style)]
        for which, perf in (("local", l.local), ("global", l.global_)):
            have[Slot("performer", f"{k}{which}.", "proj_ws")] = perf.proj_ws
            styles.append((f"{k}{which}.style.", perf.style))
        for pre, st in styles:
            have[Slot("style", pre, "out_ws")], have[Slot("style", pre, "out_ws3")] = st.out_ws, st.out_ws3
    assert {slot: p for slot, p in have.items() if p} == want


@pytest.mark.parametrize("precision", [1, 2, 4, 5])  # one per weight-format class (3 shares its planes with 1)
def test_hooks_invalidate_the_packed_cache(precision):
    """A module that has run, then gets the weights of a second seed (load_state_dict), then its ephemeral Linears
    (set_ephemerals), then its Performer projections (set_projections): after each hook the forward is a fresh module's built
    in that state -- none may leave a pack, stream or text cache of the old state in use."""
    case = "fwd_small_dims"
    _, meta, args, kw = _case(case)
    y = _fresh_out(case, precision)
    meta2 = dict(meta, wseed=meta["wseed"] + 1)
    _, eph1, proj1, _ = golden_state(meta)
    sd2, eph2, proj2, _ = golden_state(meta2)
    m, _ = build_module(meta, precision=precision)
    assert torch.equal(m(*args, **kw), y)
    steps = (("load_state_dict", lambda: m.load_state_dict(sd2, strict=True), eph1, proj1),
             ("set_ephemerals", lambda: m.set_ephemerals(eph2), eph2, proj1),
             ("set_projections", lambda: m.set_projections(proj2), eph2, proj2))
    for hook, apply, eph, proj in steps:
        f, _ = build_module(meta2, precision=precision)  # the second seed's weights, then this step's captured randomness
        f.set_ephemerals(eph), f.set_projections(proj)
        want = f(*args, **kw)
        del f
        assert not torch.equal(want, y), f"{hook}: the new state must change the forward"
        apply()
        y = m(*args, **kw)
        assert torch.equal(y, want), (f"precision {precision}, after {hook}", _differ(y, want))
