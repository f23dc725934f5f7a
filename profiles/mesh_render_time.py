#!/usr/bin/env python3
"""Time motion_render.render_mesh (csrc/motion_mesh_render.hip) on the GPU and write
profiles/mesh_render_time.txt (``--out``).

Shape: B = 32, T = 196, 480 x 480, the default ``capsule_body`` (2144 vertices) skinned on the device under a walking clip
with rotations that swing the limbs.  Configurations: RGB and palette, flat (no normals) and smooth.  Beside it, in the same
process on the same box, ``render_motion`` (§21) on the same clips' joints, for scale.  Device events around the whole call
(the host's checks, the output's and the scratch's allocation from torch's cache, the three launches); median of 9 calls after
3 warm-up calls per configuration; no profiler attached.  Recorded only; nothing is gated on it.

    timeout -k 10 600 python profiles/mesh_render_time.py
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, warm=3, calls=9):
    for _ in range(warm):
        fn()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in pairs:
        a.record()
        out = fn()
        b.record()
        del out
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def clip(MM, MF, B, T, dev):
    """Joints and global rotations of a stylised walk: forward kinematics of limbs that swing about the X axis."""
    sk = MF.get_skeleton("t2m")
    off = np.asarray(sk.raw_offsets, np.float64) * 0.25
    parents, _ = MM.pivots_of("t2m")
    J = len(parents)
    rs = np.random.RandomState(0)
    phase = rs.uniform(0, 2 * np.pi, (B, 1, J))
    ang = 0.6 * np.sin(2 * np.pi * np.arange(T)[None, :, None] / 40.0 + phase) * (np.arange(J) > 0)
    c, s, o, l = np.cos(ang), np.sin(ang), np.zeros_like(ang), np.ones_like(ang)
    local = np.stack([np.stack([l, o, o], -1), np.stack([o, c, -s], -1), np.stack([o, s, c], -1)], -2)
    R, P = np.zeros((B, T, J, 3, 3)), np.zeros((B, T, J, 3))
    P[:, :, 0] = np.stack([0.01 * np.arange(T), np.full(T, 0.95), 0.02 * np.arange(T)], -1)[None] * (1 + 0.02 * np.arange(B))[:, None, None]
    R[:, :, 0] = local[:, :, 0]
    for chain in sk.chains:
        for a, b in zip(chain[:-1], chain[1:]):
            R[:, :, b] = R[:, :, a] @ local[:, :, b]
            P[:, :, b] = P[:, :, a] + np.einsum("btij,j->bti", R[:, :, b], off[b])
    mesh = MM.capsule_body(off, "t2m")
    return mesh, torch.from_numpy(P.astype(np.float32)).to(dev), torch.from_numpy(R.astype(np.float32)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render_time.txt"))
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render_time.py measures the GPU kernels: no GPU found")
    MM = importlib.import_module("motiondiffusion-moe_amd.motion_mesh")
    MF = importlib.import_module("motiondiffusion-moe_amd.motion_features")
    MR = importlib.import_module("motiondiffusion-moe_amd.motion_render")
    L = importlib.import_module("motiondiffusion-moe_amd._lib")
    dev = torch.device("cuda:0")
    B, T, size = a.batch, 196, (480, 480)
    mesh, P, R = clip(MM, MF, B, T, dev)
    v, n = MM.skin_vertices(mesh, P, R, None, return_normals=True)
    faces = torch.from_numpy(mesh.faces).to(dev)
    V, F = mesh.n_vertices, len(mesh.faces)
    lines = [f"mdm_mesh_render (csrc/motion_mesh_render.hip) on {torch.cuda.get_device_name(0)}: wall time of motion_render.render_mesh, "
             f"device events around the whole call, no profiler attached, one process.  B = {B}, T = {T}, {size[0]} x {size[1]}, the "
             f"default capsule_body ({V} vertices, {F} faces) skinned on the device under a walking clip, default camera and style.  "
             "Median of 9 calls after 3 warm-up calls per configuration.  Beside it render_motion (§21) on the same clips' joints.  "
             "Recorded only; nothing is gated on it.", ""]
    for name, fn in (
            ("render_mesh   RGB     flat  ", lambda: MR.render_mesh(v, faces, root=P, size=size)),
            ("render_mesh   RGB     smooth", lambda: MR.render_mesh(v, faces, root=P, normals=n, size=size)),
            ("render_mesh   palette flat  ", lambda: MR.render_mesh(v, faces, root=P, size=size, palette=True)),
            ("render_mesh   palette smooth", lambda: MR.render_mesh(v, faces, root=P, normals=n, size=size, palette=True)),
            ("render_motion RGB           ", lambda: MR.render_motion(P, size=size)),
            ("render_motion palette       ", lambda: MR.render_motion(P, size=size, palette=True))):
        med, lo, hi = timed(fn)
        lines.append(f"{name}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    body = int((MR.render_mesh(v[:1, :1], faces, root=P[:1, :1], size=size)[0, 0]
                != MR.render_mesh(v[:1, :1], faces, root=P[:1, :1], size=size, body_alpha=0.0)[0, 0]).any(-1).sum())
    for normals in (0, 1):
        words = int(L.lib().mdm_mesh_render_scratch_floats(B, T, T, V, F, normals))
        lines.append(f"scratch passed to mdm_mesh_render, {'smooth' if normals else 'flat'}: {words} floats ({words * 4 / 1e6:.0f} MB)")
    lines.append(f"the body covers {body} of the {size[0] * size[1]} pixels of sample 0's first frame")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
