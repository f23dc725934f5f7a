#!/usr/bin/env python3
"""Time one whole generation at the configs[1] shape (small, 8 experts, B=32, T=196, guided, 1000-step schedule) through
DDPMTrainer.generate for the samplers it offers: guided DDPM over all 1000 steps, guided DDIM in 50 and 20 steps and
DPM-Solver++(2M) in 20 steps, at precision 1 (bf16) and 3 (fp32-grade).

A generation is the whole call: text embedding lookup, the warm-up step and graph capture of the loop, every replay, the
copy-out.  Each is timed with a host clock between two device synchronisations, after one untimed generation of the same
shape.  The two DDIM lengths split the time into a per-step part and a fixed part: step = (t50 - t20) / 30, fixed =
t20 - 20 step.  Prints one JSON line per (precision, sampler) and a table.

    timeout -k 10 900 python tools/sample_time.py [--reps 2] [--precisions 1,3]

``--edit prefix:N`` or ``--edit inbetween:H,T`` measures motion editing instead: every sampler runs the same generation
without and with that frame mask (``edit_motion``/``edit_mask``), alternating, ``--reps`` pairs after one untimed pair, and
reports both medians and the per-pair difference (median, min, max; per generation and per step).

    timeout -k 10 900 python tools/sample_time.py --edit prefix:40 --reps 5 --precisions 1

``--compose K`` measures composed guidance instead: DDIM-50 and DPM-Solver++(2M)-20 generations with K prompts per sample
(a timeline split, ``prompt_weights``) against the same plain generations, alternating, as for ``--edit``; K may be a list.

    timeout -k 10 900 python tools/sample_time.py --compose 2,3 --reps 5 --precisions 1

``--control I`` measures joint-position control instead: DDIM-50 and DPM-Solver++(2M)-20 generations steered toward target
heights of every joint on every frame (``control_joints``/``control_weights``, ``control_iters`` = I) against the same plain generations, alternating, as for
``--edit``; I may be a list.

    timeout -k 10 900 python tools/sample_time.py --control 1,5 --reps 5 --precisions 1

``--long H`` measures long-motion generation instead: the batch's windows as B / 4 long motions of four windows each,
neighbours sharing H frames (``generate_long``, eps blended and noise copied on every step), against plain generations of
the same B windows, DDIM-50 and DPM-Solver++(2M)-20, alternating, as for ``--edit``.

    timeout -k 10 900 python tools/sample_time.py --long 20 --reps 5 --precisions 1

``--control I --scene K`` measures scene constraints: the controlled generations above without and with
a scene of K primitives (spheres, pillars, boxes and floors in turn, every joint with a radius), alternating, as for ``--edit``.

    timeout -k 10 900 python tools/sample_time.py --control 1,5 --scene 4,16 --reps 5 --precisions 1

``--control I --terrain G`` measures a terrain: the controlled generations above without and with a
G x G height field and ``terrain_stand="contacts"``:

    timeout -k 10 900 python tools/sample_time.py --control 1,5 --terrain 128 --reps 5 --precisions 1

``--partners`` measures characters sampled together: 16 scenes of two characters against the same rows
with 21 static tracks and against the sequential two-stage ``generate_together``, DDIM-50 and DPM-Solver++(2M)-20:
    timeout -k 10 900 python tools/sample_time.py --partners --reps 5 --precisions 1 > profiles/partners_sample_time.txt
``--self`` measures self-collision avoidance: a controlled generation (every joint's height, ``control_iters``
1) without and with ``self_collision``, DDIM-50 and DPM-Solver++(2M)-20, alternating, as for ``--edit``:
    timeout -k 10 900 python tools/sample_time.py --self --reps 5 --precisions 1 > profiles/self_sample_time.txt
``--control I --scene K --tracks far,near,near_nobounds`` measures tracks: the controlled generation with
a scene of K primitives without and with the 21 capsule tracks of a character (``motion_scene.character_tracks``): far from the
motion (every joint outside the frames' balls), around it, and around it without the broad phase.

    timeout -k 10 900 python tools/sample_time.py --control 1,5 --scene 4 --tracks far,near,near_nobounds --reps 5 --precisions 1

``--long-control I`` (with ``--long H``, default 20) measures joint control over the canvases of those long motions: the same
``generate_long`` without and with ``control_joints`` / ``control_weights`` over every canvas frame (every joint's height,
``control_iters`` = I; I may be a list), DDIM-50 and DPM-Solver++(2M)-20, alternating, as for ``--edit``.

    timeout -k 10 900 python tools/sample_time.py --long-control 1,5 --reps 5 --precisions 1
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SAMPLERS = (("ddpm", None, 1000), ("ddim", 50, 50), ("ddim", 20, 20), ("dpmpp2m", 20, 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2, help="timed generations per sampler (the median is reported)")
    ap.add_argument("--precisions", default="1,3")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=196)
    ap.add_argument("--edit", default=None, help="prefix:N | inbetween:H,T: time editing against plain generation")
    ap.add_argument("--compose", default=None, help="K[,K...]: time K-prompt composed generation against plain")
    ap.add_argument("--control", default=None, help="I[,I...]: time joint control with I iterations against plain")
    ap.add_argument("--scene", default=None, help="K[,K...] (with --control): time a scene of K primitives against joint "
                    "control alone")
    ap.add_argument("--tracks", default=None, help="far,near,near_nobounds (with --control and --scene): time 21 character tracks "
                    "against control with the scene alone")
    ap.add_argument("--partners", action="store_true", help="time characters sampled together (16 scenes of two, 21 bones) "
                    "against 21 static character tracks and against the two-stage sequential generate_together")
    ap.add_argument("--self", dest="self_", action="store_true", help="time self-collision avoidance against the same controlled "
                    "generation without it")
    ap.add_argument("--terrain", type=int, default=None, help="G (with --control): time a G x G terrain with "
                    'terrain_stand="contacts" against joint control alone')
    ap.add_argument("--long", type=int, default=None, help="H: time long motions (4 windows each, H shared frames) "
                    "against plain generation of the same windows")
    ap.add_argument("--long-control", default=None, help="I[,I...]: time canvas joint control with I iterations against "
                    "plain long motions (overlap --long, default 20)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_time.py measures the GPU sampler: no GPU found")
    bench = importlib.import_module("bench")
    Tr = importlib.import_module("motiondiffusion-moe_amd.trainer")
    dev = torch.device("cuda:0")
    B, T = a.batch, a.frames
    m, (_, length, xf_proj, xf_out), _ = bench.build_model("small", dev, 1, B, T, 28)
    length[0] = T  # the batch runs at T frames
    m.text_encoder_fn = lambda text, device: (xf_proj[:len(text)].to(device), xf_out[:len(text)].to(device))
    import types
    tr = Tr.DDPMTrainer(types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=False, cfg_scale=7.5), m)
    caps = [f"caption {i}" for i in range(B)]
    if a.partners:
        return partners_main(a, tr, m, caps, B, T)
    if a.self_:
        return self_main(a, tr, m, caps, B, T)
    if a.edit:
        return edit_main(a, tr, m, caps, length, B, T)
    if a.compose:
        return compose_main(a, tr, m, caps, length, B, T)
    if a.control and a.scene and a.tracks:
        return tracks_main(a, tr, m, caps, length, B, T)
    if a.control and a.scene:
        return scene_main(a, tr, m, caps, length, B, T)
    if a.control and a.terrain:
        return terrain_main(a, tr, m, caps, length, B, T)
    if a.control:
        return control_main(a, tr, m, caps, length, B, T)
    if a.long_control:
        return long_control_main(a, tr, m, caps, B, T)
    if a.long is not None:
        return long_main(a, tr, m, caps, B, T)
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        res = {}
        for sampler, steps, n in SAMPLERS:
            def gen():
                return tr.generate(caps, length, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps)
            out = gen()  # warm-up: code objects, packs, caches
            assert all(torch.isfinite(o).all() for o in out)
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gen()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            ms = sorted(ts)[len(ts) // 2] * 1e3
            name = {"ddpm": "DDPM", "ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
            res[name] = ms
            line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, ms_per_generation=round(ms, 2),
                        ms_per_step=round(ms / n, 3), reps_ms=[round(t * 1e3, 2) for t in ts])
            rows.append(line)
            print(json.dumps(line), flush=True)
        step = (res["DDIM-50"] - res["DDIM-20"]) / 30
        fixed = res["DDIM-20"] - 20 * step
        line = dict(precision=prec, guided_ddim_step_ms=round(step, 3), fixed_ms_per_generation=round(fixed, 2),
                    fixed_share_at_20_steps=round(fixed / res["DPM-Solver++(2M)-20"], 3))
        rows.append(line)
        print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), 1000-step schedule; {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'sampler':>22} {'ms/generation':>14} {'ms/step':>9}")
    for r in rows:
        if "sampler" in r:
            print(f"{r['precision']:>9} {r['sampler']:>22} {r['ms_per_generation']:>14.1f} {r['ms_per_step']:>9.3f}")
        else:
            print(f"{r['precision']:>9} {'(per step | fixed)':>22} {r['fixed_ms_per_generation']:>14.1f} "
                  f"{r['guided_ddim_step_ms']:>9.3f}")


def edit_mask(spec, T):
    E = importlib.import_module("motiondiffusion-moe_amd.motion_edit")
    kind, _, arg = spec.partition(":")
    if kind == "prefix":
        return E.prefix_mask(T, int(arg))
    if kind == "inbetween":
        head, tail = (int(v) for v in arg.split(","))
        return E.inbetween_mask(T, head, tail)
    raise SystemExit(f"--edit must be prefix:N or inbetween:H,T, not {spec!r}")


def edit_main(a, tr, m, caps, length, B, T):
    dev = torch.device("cuda:0")
    mask = edit_mask(a.edit, T)
    known = torch.rand((B, T, 263), generator=torch.Generator().manual_seed(0)).to(dev) * 2 - 1
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for sampler, steps, n in SAMPLERS:
            def gen(edit):
                extra = dict(edit_motion=known, edit_mask=mask) if edit else {}
                return tr.generate(caps, length, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps, **extra)
            for edit in (False, True):  # warm-up
                assert all(torch.isfinite(o).all() for o in gen(edit))
            ts = {False: [], True: []}
            for _ in range(a.reps):
                for edit in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    gen(edit)
                    torch.cuda.synchronize()
                    ts[edit].append((time.perf_counter() - t0) * 1e3)
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            diff = sorted(e - p for p, e in zip(ts[False], ts[True]))
            name = {"ddpm": "DDPM", "ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
            line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, edit=a.edit, plain_ms=round(med[False], 2),
                        edit_ms=round(med[True], 2), diff_ms_median=round(diff[len(diff) // 2], 2),
                        diff_ms_min=round(diff[0], 2), diff_ms_max=round(diff[-1], 2),
                        diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1),
                        plain_reps_ms=[round(t, 2) for t in ts[False]], edit_reps_ms=[round(t, 2) for t in ts[True]])
            rows.append(line)
            print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), edit {a.edit}; {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'sampler':>22} {'plain ms':>9} {'edit ms':>9} {'diff ms (min..max)':>22} {'us/step':>8}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['sampler']:>22} {r['plain_ms']:>9.1f} {r['edit_ms']:>9.1f} {spread:>22} "
              f"{r['diff_us_per_step']:>8.1f}")


def compose_main(a, tr, m, caps, length, B, T):
    MC = importlib.import_module("motiondiffusion-moe_amd.motion_compose")
    xp_all, xo_all = m.text_encoder_fn(caps, torch.device("cuda:0"))  # one embedding per caption, looked up by name
    row = {c: i for i, c in enumerate(caps)}
    m.text_encoder_fn = lambda text, device: (xp_all[[row[c] for c in text]].to(device),
                                              xo_all[[row[c] for c in text]].to(device))
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for K in [int(k) for k in a.compose.split(",")]:
            w = MC.timeline_weights(T, [T * (k + 1) // K for k in range(K - 1)], blend=10)[None]
            kcaps = [tuple(caps[(i + k) % B] for k in range(K)) for i in range(B)]
            for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
                def gen(comp):
                    if comp:
                        return tr.generate(kcaps, length, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps,
                                           prompt_weights=w)
                    return tr.generate(caps, length, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps)
                for comp in (False, True):  # warm-up
                    assert all(torch.isfinite(o).all() for o in gen(comp))
                ts = {False: [], True: []}
                for _ in range(a.reps):
                    for comp in (False, True):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        gen(comp)
                        torch.cuda.synchronize()
                        ts[comp].append((time.perf_counter() - t0) * 1e3)
                med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
                name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
                line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, K=K, plain_ms=round(med[False], 2),
                            compose_ms=round(med[True], 2), ratio=round(med[True] / med[False], 3),
                            plain_reps_ms=[round(t, 2) for t in ts[False]], compose_reps_ms=[round(t, 2) for t in ts[True]])
                rows.append(line)
                print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), composed prompts; {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'K':>2} {'sampler':>22} {'plain ms':>9} {'composed ms':>12} {'ratio':>6} {'(K+1)/2':>8}")
    for r in rows:
        print(f"{r['precision']:>9} {r['K']:>2} {r['sampler']:>22} {r['plain_ms']:>9.1f} {r['compose_ms']:>12.1f} "
              f"{r['ratio']:>6.2f} {(r['K'] + 1) / 2:>8.1f}")


def control_main(a, tr, m, caps, length, B, T):
    # every joint's height on every frame: the densest weight map (every steerable column is written on every iteration),
    # and a loss quadratic in x0, so the unclipped random-weight samples stay finite at any step size used here
    tg, w = torch.zeros(B, T, 22, 3), torch.zeros(B, T, 22, 3)
    tg[..., 1], w[..., 1] = 1.0, 1.0
    mean, std = torch.zeros(263), torch.ones(263)
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for iters in [int(k) for k in a.control.split(",")]:
            for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
                def gen(ctl):
                    extra = dict(control_joints=tg, control_weights=w, control_scale=0.05, control_iters=iters,
                                 mean=mean, std=std) if ctl else {}
                    return tr.generate(caps, length, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps,
                                       **extra)
                for ctl in (False, True):  # warm-up
                    assert all(torch.isfinite(o).all() for o in gen(ctl))
                ts = {False: [], True: []}
                for _ in range(a.reps):
                    for ctl in (False, True):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        gen(ctl)
                        torch.cuda.synchronize()
                        ts[ctl].append((time.perf_counter() - t0) * 1e3)
                med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
                diff = sorted(c - p for p, c in zip(ts[False], ts[True]))
                name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
                line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, control_iters=iters,
                            plain_ms=round(med[False], 2), control_ms=round(med[True], 2),
                            diff_ms_median=round(diff[len(diff) // 2], 2), diff_ms_min=round(diff[0], 2),
                            diff_ms_max=round(diff[-1], 2), diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1),
                            plain_reps_ms=[round(t, 2) for t in ts[False]], control_reps_ms=[round(t, 2) for t in ts[True]])
                rows.append(line)
                print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), joint control (every joint's height); {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'iters':>5} {'sampler':>22} {'plain ms':>9} {'control ms':>11} {'diff ms (min..max)':>22} "
          f"{'us/step':>8}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['control_iters']:>5} {r['sampler']:>22} {r['plain_ms']:>9.1f} "
              f"{r['control_ms']:>11.1f} {spread:>22} {r['diff_us_per_step']:>8.1f}")


def scene_main(a, tr, m, caps, length, B, T):
    # the controlled generation of control_main, without and with a scene: keep-out primitives of every kind in turn (their
    # force is bounded by their size, so the unclipped random-weight samples stay finite) around the origin
    MS = importlib.import_module("motiondiffusion-moe_amd.motion_scene")
    tg, w = torch.zeros(B, T, 22, 3), torch.zeros(B, T, 22, 3)
    tg[..., 1], w[..., 1] = 1.0, 1.0
    mean, std = torch.zeros(263), torch.ones(263)

    def scene_of(K):
        out = []
        for k in range(K):
            x, z = 0.8 * (k % 4) - 1.2, 0.8 * (k // 4) - 1.2
            out.append([MS.sphere((x, 1.0, z), 0.4, margin=0.05), MS.capsule((x, 0.0, z), (x, 2.0, z), 0.2),
                        MS.box((x, 0.5, z), (0.3, 0.5, 0.2), 0.3 * k), MS.floor(-0.1 * k)][k % 4])
        return out

    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for iters in [int(k) for k in a.control.split(",")]:
            for K in [int(k) for k in a.scene.split(",")]:
                scene = scene_of(K)
                for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
                    def gen(sc):
                        extra = dict(scene=scene, scene_joint_radius=[0.05] * 22) if sc else {}
                        return tr.generate(caps, length, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps,
                                           control_joints=tg, control_weights=w, control_scale=0.05, control_iters=iters,
                                           mean=mean, std=std, **extra)
                    for sc in (False, True):  # warm-up
                        assert all(torch.isfinite(o).all() for o in gen(sc))
                    ts = {False: [], True: []}
                    for _ in range(a.reps):
                        for sc in (False, True):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            gen(sc)
                            torch.cuda.synchronize()
                            ts[sc].append((time.perf_counter() - t0) * 1e3)
                    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
                    diff = sorted(c - p for p, c in zip(ts[False], ts[True]))
                    name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
                    line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, control_iters=iters, prims=K,
                                control_ms=round(med[False], 2), scene_ms=round(med[True], 2),
                                diff_ms_median=round(diff[len(diff) // 2], 2), diff_ms_min=round(diff[0], 2),
                                diff_ms_max=round(diff[-1], 2), diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1),
                                control_reps_ms=[round(t, 2) for t in ts[False]], scene_reps_ms=[round(t, 2) for t in ts[True]])
                    rows.append(line)
                    print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), joint control (every joint's height) without and with a scene; "
          f"{torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'iters':>5} {'prims':>5} {'sampler':>22} {'control ms':>11} {'scene ms':>9} {'diff ms (min..max)':>22} "
          f"{'us/step':>8}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['control_iters']:>5} {r['prims']:>5} {r['sampler']:>22} {r['control_ms']:>11.1f} "
              f"{r['scene_ms']:>9.1f} {spread:>22} {r['diff_us_per_step']:>8.1f}")


def terrain_main(a, tr, m, caps, length, B, T):
    # the controlled generation of control_main, without and with a terrain of G x G samples: rolling
    # ground of 0.25 m cells centred on the origin, 0.3 m high, so that joints lie under and over it and walk across its cells;
    # the stand weights come from every step's own contact labels.  The term is quadratic in a joint's height, as the targets'.
    MS = importlib.import_module("motiondiffusion-moe_amd.motion_scene")
    tg, w = torch.zeros(B, T, 22, 3), torch.zeros(B, T, 22, 3)
    tg[..., 1], w[..., 1] = 1.0, 1.0
    mean, std = torch.zeros(263), torch.ones(263)
    G, cell = a.terrain, 0.25
    i = torch.arange(G, dtype=torch.float64) * cell
    ground = MS.heightfield(0.3 * torch.sin(i[None] * 0.7) * torch.cos(i[:, None] * 0.5), cell,
                            (-0.5 * (G - 1) * cell, -0.5 * (G - 1) * cell), 0.3, margin=0.02)
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for iters in [int(k) for k in a.control.split(",")]:
            for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
                def gen(on):
                    extra = dict(terrain=ground, terrain_stand="contacts", scene_joint_radius=[0.05] * 22) if on else {}
                    return tr.generate(caps, length, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps,
                                       control_joints=tg, control_weights=w, control_scale=0.05, control_iters=iters,
                                       mean=mean, std=std, **extra)
                for on in (False, True):  # warm-up
                    assert all(torch.isfinite(o).all() for o in gen(on))
                ts = {False: [], True: []}
                for _ in range(a.reps):
                    for on in (False, True):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        gen(on)
                        torch.cuda.synchronize()
                        ts[on].append((time.perf_counter() - t0) * 1e3)
                med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
                diff = sorted(c - p for p, c in zip(ts[False], ts[True]))
                name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
                line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, control_iters=iters, grid=G,
                            control_ms=round(med[False], 2), terrain_ms=round(med[True], 2),
                            diff_ms_median=round(diff[len(diff) // 2], 2), diff_ms_min=round(diff[0], 2),
                            diff_ms_max=round(diff[-1], 2), diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1),
                            control_reps_ms=[round(t, 2) for t in ts[False]], terrain_reps_ms=[round(t, 2) for t in ts[True]])
                rows.append(line)
                print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), joint control (every joint's height) without and with a "
          f"{G} x {G} terrain, terrain_stand=\"contacts\"; {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'iters':>5} {'sampler':>22} {'control ms':>11} {'terrain ms':>11} {'diff ms (min..max)':>22} {'us/step':>8}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['control_iters']:>5} {r['sampler']:>22} {r['control_ms']:>11.1f} "
              f"{r['terrain_ms']:>11.1f} {spread:>22} {r['diff_us_per_step']:>8.1f}")


def tracks_main(a, tr, m, caps, length, B, T):
    # scene_main's generation with its scene, without and with the 21 capsule tracks of a character.  The unclipped
    # random-weight samples are hundreds of metres across, so the character "around the motion" is a cloud of that size (every
    # joint inside the frames' balls: every record is walked; thin capsules, so the forces stay bounded) and the one "far from
    # it" the same cloud 1e6 m away (every joint outside: the broad phase skips every frame).
    MS = importlib.import_module("motiondiffusion-moe_amd.motion_scene")
    tg, w = torch.zeros(B, T, 22, 3), torch.zeros(B, T, 22, 3)
    tg[..., 1], w[..., 1] = 1.0, 1.0
    mean, std = torch.zeros(263), torch.ones(263)
    K = int(a.scene.split(",")[0])
    scene = []
    for k in range(K):
        x, z = 0.8 * (k % 4) - 1.2, 0.8 * (k // 4) - 1.2
        scene.append([MS.sphere((x, 1.0, z), 0.4, margin=0.05), MS.capsule((x, 0.0, z), (x, 2.0, z), 0.2),
                      MS.box((x, 0.5, z), (0.3, 0.5, 0.2), 0.3 * k), MS.floor(-0.1 * k)][k % 4])
    gen_ = torch.Generator().manual_seed(0)
    cloud = torch.randn(1, 22, 3, generator=gen_, dtype=torch.float64) * 300 + torch.cumsum(
        torch.randn(T, 1, 3, generator=gen_, dtype=torch.float64) * 5, 0)
    bounds_of = MS.track_bounds

    def no_bounds(rec):
        out = bounds_of(rec)
        out[..., 3] = float("inf")
        return out

    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for iters in [int(k) for k in a.control.split(",")]:
            for case in a.tracks.split(","):
                shift = torch.tensor([1e6, 0.0, 0.0], dtype=torch.float64) if case == "far" else 0.0
                tracks = MS.character_tracks(cloud + shift, 0.08, margin=0.05)
                MS.track_bounds = no_bounds if case.endswith("nobounds") else bounds_of
                for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
                    def gen(trk):
                        extra = dict(scene_tracks=tracks) if trk else {}
                        return tr.generate(caps, length, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps,
                                           control_joints=tg, control_weights=w, control_scale=0.05, control_iters=iters,
                                           mean=mean, std=std, scene=scene, scene_joint_radius=[0.05] * 22, **extra)
                    for trk in (False, True):  # warm-up
                        assert all(torch.isfinite(o).all() for o in gen(trk))
                    ts = {False: [], True: []}
                    for _ in range(a.reps):
                        for trk in (False, True):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            gen(trk)
                            torch.cuda.synchronize()
                            ts[trk].append((time.perf_counter() - t0) * 1e3)
                    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
                    diff = sorted(c - p for p, c in zip(ts[False], ts[True]))
                    name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
                    line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, control_iters=iters, prims=K, tracks=case,
                                scene_ms=round(med[False], 2), tracks_ms=round(med[True], 2),
                                diff_ms_median=round(diff[len(diff) // 2], 2), diff_ms_min=round(diff[0], 2),
                                diff_ms_max=round(diff[-1], 2), diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1),
                                scene_reps_ms=[round(t, 2) for t in ts[False]], tracks_reps_ms=[round(t, 2) for t in ts[True]])
                    rows.append(line)
                    print(json.dumps(line), flush=True)
    MS.track_bounds = bounds_of
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), joint control (every joint's height) with a scene of {K} primitives, "
          f"without and with 21 character tracks; {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'iters':>5} {'tracks':>14} {'sampler':>22} {'scene ms':>9} {'tracks ms':>10} {'diff ms (min..max)':>22} "
          f"{'us/step':>8}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['control_iters']:>5} {r['tracks']:>14} {r['sampler']:>22} {r['scene_ms']:>9.1f} "
              f"{r['tracks_ms']:>10.1f} {spread:>22} {r['diff_us_per_step']:>8.1f}")


def partners_main(a, tr, m, caps, B, T):
    # B / 2 scenes of two characters sampled together, in alternating pairs against (a) the same rows with
    # 21 static "near" character tracks (tracks_main's cloud around the samples): what the producer launch costs on top of the
    # guidance it feeds, and (b) the two-stage sequential generate_together: two generations of B / 2 rows against one of B.
    MS = importlib.import_module("motiondiffusion-moe_amd.motion_scene")
    if B % 2:
        raise SystemExit("--partners needs a batch of whole two-character scenes")
    # The unclipped random-weight samples are rows of size thousands: the de-normalisation scales them down (std 0.002 for the
    # root velocities and the height, 0.0005 for the joint columns, 1e-4 for the heading velocity; the "bodies" are still
    # clouds that wander hundreds of metres), and the step and the avoidance weight are small, so that the guidance stays
    # finite over 196 frames (the warm-up asserts it).  The cost does not depend on the weight.  The static tracks are
    # tracks_main's "near" cloud, of the samples' own extent: most joints are inside the frames' balls and walk all 21 records.
    mean, std = torch.zeros(263), torch.full((263,), 0.002)
    std[0], std[4:67] = 1e-4, 0.0005
    tg, w = torch.zeros(T, 22, 3), torch.zeros(T, 22)
    tg[..., 1], w[:] = 1.0, 1.0  # every joint's height, as tracks_main: all modes run the guidance with targets
    scenes = [[dict(caption=caps[2 * i], length=T, control_joints=tg, control_weights=w),
               dict(caption=caps[2 * i + 1], length=T, position=(0.5, 0.0), yaw=0.3, control_joints=tg, control_weights=w)]
              for i in range(B // 2)]
    gen_ = torch.Generator().manual_seed(0)
    cloud = torch.randn(1, 22, 3, generator=gen_, dtype=torch.float64) * 300 + torch.cumsum(
        torch.randn(T, 1, 3, generator=gen_, dtype=torch.float64) * 5, 0)
    tracks = MS.character_tracks(cloud, 0.08, margin=0.05, weight=0.01)
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
            opts = dict(seed=0, sampler=sampler, sample_steps=steps, control_scale=5.0, control_iters=1, sigma=0.0, batch_size=B)
            pair = dict(radius=0.08, margin=0.05, weight=0.01)
            runs = {"mutual": lambda: tr.generate_together(scenes, 263, mean, std, mutual=True, **pair, **opts),
                    "static": lambda: tr.generate_joints(caps, torch.full((B,), T), 263, mean, std, scene_tracks=tracks,
                                                         control_joints=tg[None].expand(B, -1, -1, -1),
                                                         control_weights=w[None].expand(B, -1, -1), **opts),
                    "sequential": lambda: tr.generate_together(scenes, 263, mean, std, **pair, **opts)}
            for other in ("static", "sequential"):
                for k in ("mutual", other):  # warm-up
                    res = runs[k]()
                    assert all(torch.isfinite(j).all() for v in res for j in (v if isinstance(v, list) else [v])), k
                ts = {"mutual": [], other: []}
                for _ in range(a.reps):
                    for k in (other, "mutual"):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        runs[k]()
                        torch.cuda.synchronize()
                        ts[k].append((time.perf_counter() - t0) * 1e3)
                med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
                diff = sorted(c - p for p, c in zip(ts[other], ts["mutual"]))
                name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
                line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, against=other, other_ms=round(med[other], 2),
                            mutual_ms=round(med["mutual"], 2), diff_ms_median=round(diff[len(diff) // 2], 2),
                            diff_ms_min=round(diff[0], 2), diff_ms_max=round(diff[-1], 2),
                            diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1),
                            other_reps_ms=[round(t, 2) for t in ts[other]], mutual_reps_ms=[round(t, 2) for t in ts["mutual"]])
                rows.append(line)
                print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}: {B // 2} scenes of two characters sampled together (21 bones, control_iters 1) against "
          f"the same rows with 21 static near tracks and against the sequential generate_together; {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'against':>11} {'sampler':>22} {'other ms':>9} {'mutual ms':>10} {'diff ms (min..max)':>22} {'us/step':>8}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['against']:>11} {r['sampler']:>22} {r['other_ms']:>9.1f} {r['mutual_ms']:>10.1f} {spread:>22} "
              f"{r['diff_us_per_step']:>8.1f}")


def self_main(a, tr, m, caps, B, T):
    # The same controlled generation (every joint's height as a target, as partners_main: both modes run the guidance with
    # targets) without and with self_collision, in alternating pairs: what the producer (the two launches of
    # the joints and the push launch, every step) costs on top of the guidance it feeds.  The de-normalisation, the step and the
    # small weight are partners_main's, for the same reason: the unclipped random-weight samples are clouds, and the warm-up
    # asserts finite results; the cost does not depend on the weight.
    mean, std = torch.zeros(263), torch.full((263,), 0.002)
    std[0], std[4:67] = 1e-4, 0.0005
    tg, w = torch.zeros(B, T, 22, 3), torch.zeros(B, T, 22)
    tg[..., 1], w[:] = 1.0, 1.0
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
            opts = dict(seed=0, sampler=sampler, sample_steps=steps, control_scale=5.0, control_iters=1, sigma=0.0, batch_size=B,
                        control_joints=tg, control_weights=w)

            def gen(own):
                return tr.generate_joints(caps, torch.full((B,), T), 263, mean, std,
                                          self_collision=dict(weight=0.01) if own else None, **opts)
            for own in (False, True):  # warm-up
                assert all(torch.isfinite(j).all() for j in gen(own)), own
            ts = {False: [], True: []}
            for _ in range(a.reps):
                for own in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    gen(own)
                    torch.cuda.synchronize()
                    ts[own].append((time.perf_counter() - t0) * 1e3)
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            diff = sorted(c - p for p, c in zip(ts[False], ts[True]))
            name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
            line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, plain_ms=round(med[False], 2), self_ms=round(med[True], 2),
                        diff_ms_median=round(diff[len(diff) // 2], 2), diff_ms_min=round(diff[0], 2), diff_ms_max=round(diff[-1], 2),
                        diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1), plain_reps_ms=[round(t, 2) for t in ts[False]],
                        self_reps_ms=[round(t, 2) for t in ts[True]])
            rows.append(line)
            print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}: joint control (every joint's height, control_iters 1) without and with self_collision "
          f"(22 joints x 21 bones, default mask); {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'sampler':>22} {'plain ms':>9} {'self ms':>9} {'diff ms (min..max)':>22} {'us/step':>8}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['sampler']:>22} {r['plain_ms']:>9.1f} {r['self_ms']:>9.1f} {spread:>22} {r['diff_us_per_step']:>8.1f}")


def long_main(a, tr, m, caps, B, T):
    if B % 4:
        raise SystemExit("--long needs a batch of whole 4-window motions")
    h = a.long
    scripts = [[(caps[4 * i + k], T) for k in range(4)] for i in range(B // 4)]
    full = torch.full((B,), T)
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
            def gen(long):
                if long:
                    return tr.generate_long(scripts, 263, overlap=h, batch_size=B, seed=0, sampler=sampler,
                                            sample_steps=steps)
                return tr.generate(caps, full, 263, batch_size=B, seed=0, sampler=sampler, sample_steps=steps)
            for long in (False, True):  # warm-up
                assert all(torch.isfinite(o).all() for o in gen(long))
            ts = {False: [], True: []}
            for _ in range(a.reps):
                for long in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    gen(long)
                    torch.cuda.synchronize()
                    ts[long].append((time.perf_counter() - t0) * 1e3)
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            diff = sorted(c - p for p, c in zip(ts[False], ts[True]))
            name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
            line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, overlap=h, motions=B // 4,
                        canvas_frames=4 * T - 3 * h, plain_ms=round(med[False], 2), long_ms=round(med[True], 2),
                        diff_ms_median=round(diff[len(diff) // 2], 2), diff_ms_min=round(diff[0], 2),
                        diff_ms_max=round(diff[-1], 2), diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1),
                        diff_share=round(diff[len(diff) // 2] / med[False], 4),
                        plain_reps_ms=[round(t, 2) for t in ts[False]], long_reps_ms=[round(t, 2) for t in ts[True]])
            rows.append(line)
            print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), {B // 4} long motions of 4 windows, overlap {h}; "
          f"{torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'sampler':>22} {'plain ms':>9} {'long ms':>9} {'diff ms (min..max)':>22} {'us/step':>8} "
          f"{'share':>7}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['sampler']:>22} {r['plain_ms']:>9.1f} {r['long_ms']:>9.1f} {spread:>22} "
              f"{r['diff_us_per_step']:>8.1f} {r['diff_share']:>7.2%}")


def long_control_main(a, tr, m, caps, B, T):
    if B % 4:
        raise SystemExit("--long-control needs a batch of whole 4-window motions")
    h = 20 if a.long is None else a.long
    C = 4 * T - 3 * h
    scripts = [[(caps[4 * i + k], T) for k in range(4)] for i in range(B // 4)]
    # every joint's height on every canvas frame: as --control, over the canvas
    tg, w = [torch.zeros(C, 22, 3) for _ in scripts], [torch.zeros(C, 22, 3) for _ in scripts]
    for g_, w_ in zip(tg, w):
        g_[..., 1], w_[..., 1] = 1.0, 1.0
    mean, std = torch.zeros(263), torch.ones(263)
    rows = []
    for prec in [int(p) for p in a.precisions.split(",")]:
        m.precision = prec
        m.invalidate()
        for iters in [int(k) for k in a.long_control.split(",")]:
            for sampler, steps, n in (("ddim", 50, 50), ("dpmpp2m", 20, 20)):
                def gen(ctl):
                    extra = dict(control_joints=tg, control_weights=w, control_scale=0.05, control_iters=iters,
                                 mean=mean, std=std) if ctl else {}
                    return tr.generate_long(scripts, 263, overlap=h, batch_size=B, seed=0, sampler=sampler,
                                            sample_steps=steps, **extra)
                for ctl in (False, True):  # warm-up
                    assert all(torch.isfinite(o).all() for o in gen(ctl))
                ts = {False: [], True: []}
                for _ in range(a.reps):
                    for ctl in (False, True):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        gen(ctl)
                        torch.cuda.synchronize()
                        ts[ctl].append((time.perf_counter() - t0) * 1e3)
                med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
                diff = sorted(c - p for p, c in zip(ts[False], ts[True]))
                name = {"ddim": "DDIM", "dpmpp2m": "DPM-Solver++(2M)"}[sampler] + f"-{n}"
                line = dict(precision=prec, sampler=name, steps=n, B=B, T=T, overlap=h, motions=B // 4, canvas_frames=C,
                            control_iters=iters, plain_ms=round(med[False], 2), control_ms=round(med[True], 2),
                            diff_ms_median=round(diff[len(diff) // 2], 2), diff_ms_min=round(diff[0], 2),
                            diff_ms_max=round(diff[-1], 2), diff_us_per_step=round(diff[len(diff) // 2] / n * 1e3, 1),
                            plain_reps_ms=[round(t, 2) for t in ts[False]], control_reps_ms=[round(t, 2) for t in ts[True]])
                rows.append(line)
                print(json.dumps(line), flush=True)
    print(f"\nconfigs[1] shape B={B} T={T}, guided (cfg 7.5), {B // 4} long motions of 4 windows, overlap {h} ({C}-frame "
          f"canvases), joint control over the canvas (every joint's height); {torch.cuda.get_device_name(0)}")
    print(f"{'precision':>9} {'iters':>5} {'sampler':>22} {'plain ms':>9} {'control ms':>11} {'diff ms (min..max)':>22} "
          f"{'us/step':>8}")
    for r in rows:
        spread = f"{r['diff_ms_median']:+.2f} ({r['diff_ms_min']:+.2f}..{r['diff_ms_max']:+.2f})"
        print(f"{r['precision']:>9} {r['control_iters']:>5} {r['sampler']:>22} {r['plain_ms']:>9.1f} "
              f"{r['control_ms']:>11.1f} {spread:>22} {r['diff_us_per_step']:>8.1f}")


if __name__ == "__main__":
    main()
