"""Host: packing.stream_plan() -- which weight stream is packed for which matrix, width and precision, and which struct field
receives it -- against tests/golden/stream_plan.json, recorded on a GPU from the PackedModel of the commit before the plan existed
(what it packed, and the tensor each struct pointer resolved to).  A stream that is planned for the wrong precision, or planned and
sent to the wrong field, drops a kernel to its slower path without changing any result: only this listing notices."""
import json
import os

import pytest
import torch

from conftest import GOLDEN, load_golden, pkg

CASES = ["fwd_tiny", "fwd_small_dims", "fwd_big_dims"]  # D = 64 (no stream in any precision), 512, 1024
PRECS = (1, 2, 3, 4, 5)
EXPERTS = ("w1", "w2")
PAIR_KINDS = ("style3", "expert3")
FIELDS = {"packed": ("ws",), "style": ("out_ws", "out_ws3"), "performer": ("proj_ws",), "layer": ("wstream", "sd_ffn_ws")}

with open(os.path.join(GOLDEN, "stream_plan.json")) as _f:
    RECORDED = json.load(_f)


def _cfg(case):
    meta = load_golden(case)[1]
    c = meta["cfg"]
    D, F, Dt = pkg("layout").resolve_dims(c["latent_dim_arg"], c["ff_size_arg"], c["text_latent_dim_arg"], c["model_size"])
    return dict(latent_dim=D, ff_size=F, text_latent_dim=Dt, num_heads=c["num_heads"], num_layers=c["num_layers"],
                moe_num_experts=c["moe_num_experts"], input_feats=c["input_feats"], num_frames=c["num_frames"])


def _leaf(name):
    return name.rsplit(".", 1)[1]


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("case", CASES)
def test_plan_matches_what_the_parent_packed(case, precision):
    ops, packing = pkg("ops"), pkg("packing")
    cfg = _cfg(case)
    assert cfg == RECORDED[case]["cfg"]  # the recorded module's kernel_cfg()
    got = {}
    for s in packing.stream_plan(cfg, precision):
        n = ops.stream_elems(s.kind, *s.shape)  # the library's own size query: entries it refuses (<= 0) are not packed
        if n > 0:
            got[s.kind, s.sources, s.slot.struct, s.slot.owner, s.slot.field] = ({"f16": "float16", "bf16": "bfloat16"}[s.h16], n)
    want = {(r["kind"], tuple(r["sources"]), r["struct"], r["owner"], r["field"]): (r["dtype"], r["numel"])
            for r in RECORDED[case][str(precision)]}
    assert len(want) == len(RECORDED[case][str(precision)])
    assert got == want, (sorted(set(got) ^ set(want)), [k for k in set(got) & set(want) if got[k] != want[k]])
    if case == "fwd_tiny":
        assert not packing.stream_plan(cfg, precision)


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("case", CASES)
def test_plan_structure(case, precision):
    L, packing = pkg("_lib"), pkg("packing")
    cfg = _cfg(case)
    head_dim = cfg["latent_dim"] // cfg["num_heads"]
    plan = packing.stream_plan(cfg, precision)
    assert len({s.key for s in plan}) == len(plan), "keys are unique"
    assert len({s.slot for s in plan}) == len(plan), "no two streams share a struct field"
    for s in plan:
        assert s.kind in packing.STREAM_KINDS and s.slot.field in FIELDS[s.slot.struct], s
        assert len(s.sources) == len(s.shape) == (2 if s.kind == "mlp" else 1), s
        assert s.h16 in ("f16", "bf16")
        if s.kind == "frag":
            assert _leaf(s.sources[0]) not in EXPERTS, "no expert matrix has a fragment stream"
        if s.kind in PAIR_KINDS:
            assert s.h16 == "bf16"
            assert all(packing.weight_format(n, precision, head_dim) == "bf16x2" for n in s.sources), s
    if precision == L.PREC_MIXED:
        assert not [s for s in plan if s.kind == "style" or s.slot.field == "proj_ws"]


@pytest.mark.parametrize("case", CASES)
def test_plan_shapes_are_views_of_the_layout(case):
    """The plan is made without tensors: the [G, N, K] views it names must be views of what kernel_layout() really produces."""
    packing, synth = pkg("packing"), pkg("synth")
    c, cfg = load_golden(case)[1]["cfg"], _cfg(case)
    D, Dt, nl, dh = cfg["latent_dim"], cfg["text_latent_dim"], cfg["num_layers"], cfg["latent_dim"] // cfg["num_heads"]

    def blank(*shape):  # only the shapes matter: one uninitialised byte per element
        return torch.empty(shape, dtype=torch.uint8)

    sd = {k: blank(*shape) for k, shape in pkg("layout").state_dict_layout(
        c["input_feats"], num_frames=c["num_frames"], latent_dim=c["latent_dim_arg"], ff_size=c["ff_size_arg"],
        num_layers=nl, num_heads=c["num_heads"], text_latent_dim=c["text_latent_dim_arg"],
        moe_num_experts=c["moe_num_experts"], model_size=c["model_size"])}
    eph = {n: ((blank(D, Dt), blank(D)) if n == "text_proj" else (blank(4 * D, D), blank(4 * D)))
           for n in synth.ephemeral_names(nl, Dt != D)}
    proj = {n: blank(dh, min(dh, 256)) for n in synth.projection_names(nl)}
    lay = {k: tuple(v.shape) for k, v in packing.kernel_layout(sd, cfg, eph, proj).items()}
    seen = 0
    for precision in PRECS:
        for s in packing.stream_plan(cfg, precision):
            for name, (G, N, K) in zip(s.sources, s.shape):
                assert lay["W:" + name] == (G * N, K), (s.key, name, lay["W:" + name])
                seen += 1
    assert seen or case == "fwd_tiny"
