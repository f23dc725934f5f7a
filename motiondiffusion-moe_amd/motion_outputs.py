"""The output chain of generated motions: rows -> joints -> rotations -> BVH or a skinned mesh and its glTF, and joints ->
frames -> GIF; what the output methods of ``DDPMTrainer`` run on the motions ``generate``, ``generate_bucketed`` or
``generate_long`` returned.  ``joints_batch`` keeps the zero-padded batch the kernels work on: ``to_joints`` slices it per
motion, ``to_bvh``, ``to_meshes`` and ``to_glb`` hand it on as it is.
"""
from __future__ import annotations

import torch
from torch.nn.utils.rnn import pad_sequence

from .motion_features import pad_clips, skeleton_for_feats
from .motion_mesh import capsule_body, glb_bytes, skin_vertices
from .motion_render import gif_bytes, render_mesh, render_motion, render_world, write_gif
from .motion_rig import DEFAULT_FPS, bvh_text, retarget_to_rig, retime_ratio, rig_of, rotations_to_rig, target_bvh_text
from .motion_rig import target_rig as make_target_rig
from .postprocess import fk_max_frames, motion_to_joints, motion_to_joints_fk, pin_limbs, remove_foot_skate

MAX_JOINTS_FRAMES = 3276  # frames of mdm_motion_postprocess: 5 T floats of LDS per workgroup, 64 KiB


def valid_lengths(motions, m_lens=None):
    """Every generated motion's ``m_lens`` entry, at most the frames it has; without ``m_lens`` all it has."""
    if m_lens is None:
        return [mo.shape[0] for mo in motions]
    return [min(int(n), mo.shape[0]) for n, mo in zip(torch.as_tensor(m_lens).flatten().tolist(), motions)]


def check_paths(paths, n, what):
    if paths is not None and len(paths) != n:
        raise ValueError(f"paths must hold one entry per {what} ({n}), or None")


def canvas_frame_limit(forward_kinematics=False):
    """The longest canvas the long variants take: with forward kinematics (``from_rotations``, BVH) ``fk_max_frames()``."""
    return fk_max_frames() if forward_kinematics else MAX_JOINTS_FRAMES


def pin_pair(pin, B, T, J):
    """``pin=`` of ``joints_batch``: (targets (N, T', J, 3), weights broadcastable to it as ``control_weights`` are), or one
    (T'_i, J, 3) target array and weights aligned on its frame dim per motion (canvases) -> (targets, weights) float32
    (B, T, J, 3) on the CPU: frames past T cut, missing frames under weight 0.  Raises ValueError."""
    from .conditioning import expand_to
    if not isinstance(pin, (tuple, list)) or len(pin) != 2 or pin[0] is None or pin[1] is None:
        raise ValueError("pin is a (targets, weights) pair")
    g, w = pin
    if not torch.is_tensor(g) and isinstance(g, (tuple, list)):  # one canvas per motion
        if isinstance(w, torch.Tensor) or len(g) != B or len(w) != B:
            raise ValueError(f"pin: one target array and one weight array per motion ({B})")
        pairs = [pin_pair((torch.as_tensor(a)[None], torch.as_tensor(b)[None]), 1, T, J) for a, b in zip(g, w)]
        return torch.cat([a for a, _ in pairs]), torch.cat([b for _, b in pairs])
    g = torch.as_tensor(g).detach().to("cpu", torch.float32)
    if g.dim() != 4 or g.shape[0] != B or tuple(g.shape[2:]) != (J, 3):
        raise ValueError(f"pin targets of shape {tuple(g.shape)} must be ({B}, T, {J}, 3)")
    w = expand_to(torch.as_tensor(w).detach().to("cpu", torch.float32), 1, g.shape, "pin weights", f"must lead with {B}")
    n = min(T, g.shape[1])
    go, wo = torch.zeros(B, T, J, 3), torch.zeros(B, T, J, 3)
    go[:, :n], wo[:, :n] = g[:, :n], w[:, :n]
    return go, wo


def pin_of(pin_targets, kw):
    """``pin_targets=`` of the trainer's output methods: None when off, else the call's own ``control_joints`` /
    ``control_weights`` out of its keyword arguments; ValueError without them."""
    if not pin_targets:
        return None
    if kw.get("control_joints") is None or kw.get("control_weights") is None:
        raise ValueError("pin_targets=True pins the call's own control_joints / control_weights: give both")
    return kw["control_joints"], kw["control_weights"]


def pin_kw(pin, pin_blend=5):
    """The keyword arguments that hand a pin on: none when there is none, so that a call without pins is the call it was."""
    return {} if pin is None else dict(pin=pin, pin_blend=pin_blend)


def joints_batch(motions, lens, dim_pose, mean, std, joints_num, sigma, from_rotations=False, offsets=None,
                 return_rotations=False, fix_feet=False, blend=5, *, pin=None, pin_blend=5):
    """``postprocess.motion_to_joints`` over the first ``lens[i]`` frames of every motion, or with ``from_rotations``
    ``postprocess.motion_to_joints_fk``: one launch for all.  -> (joints (B, T, J, 3), rotations (B, T, J, 3, 3), offsets
    (B, J, 3), lens), zero past each length; rotations and offsets are None without forward kinematics.  ``fix_feet``:
    ``postprocess.remove_foot_skate`` on the result, filtered first (filtering afterwards would smear the pins), labels from
    the rows' contact columns read in place; rotations go through it, so that joints and rotations still agree.
    ``pin``: a (targets, weights) pair over the padded batch, ``control_joints`` / ``control_weights`` as the call took them;
    ``postprocess.pin_limbs`` with ``pin_blend`` runs last: temporal filter -> ``fix_feet`` -> pins, so
    that nothing smears a pin, and where a foot-skate pin and a target both touch an ankle the target wins."""
    skel = skeleton_for_feats(dim_pose)
    if pin is not None and (skel is None or dim_pose != 12 * joints_num - 1):
        raise ValueError(f"pin needs dim_pose 263 (22 joints) or 251 (21), not {dim_pose} ({joints_num})")
    if fix_feet and (skel is None or dim_pose != 12 * joints_num - 1):
        raise ValueError(f"fix_feet needs dim_pose 263 (22 joints) or 251 (21), not {dim_pose} ({joints_num})")
    if (offsets is not None or return_rotations) and not from_rotations:
        raise ValueError("offsets and rotations belong to forward kinematics: pass from_rotations=True")
    x = pad_sequence(list(motions), batch_first=True)  # (B, longest, dim_pose), zero past each motion
    if not from_rotations:
        j = motion_to_joints(x, mean, std, torch.tensor(lens), joints_num, sigma)
        if fix_feet:
            j = remove_foot_skate(j, torch.tensor(lens), (x, mean, std), skeleton=skel, blend=blend)
        if pin is not None:
            j = pin_limbs(j, torch.tensor(lens), *pin_pair(pin, x.shape[0], x.shape[1], joints_num), skeleton=skel, blend=pin_blend)
        return j, None, None, lens
    if dim_pose != 12 * joints_num - 1 or dim_pose not in (263, 251):
        raise ValueError(f"forward kinematics needs dim_pose 263 (22 joints) or 251 (21), not {dim_pose} ({joints_num})")
    if isinstance(offsets, (list, tuple)):
        offsets = torch.stack([torch.as_tensor(o).to("cpu", torch.float32) for o in offsets])
    j, r, o = motion_to_joints_fk(x, mean, std, torch.tensor(lens), offsets, skeleton=skel, sigma=sigma,
                                  return_rotations=True, return_offsets=True)
    if fix_feet:
        j, r = remove_foot_skate(j, torch.tensor(lens), (x, mean, std), skeleton=skel, blend=blend, rotations=r)
    if pin is not None:
        j, r = pin_limbs(j, torch.tensor(lens), *pin_pair(pin, x.shape[0], x.shape[1], joints_num), skeleton=skel,
                         blend=pin_blend, rotations=r)
    return j, r, o, lens


def to_joints(motions, lens, dim_pose, mean, std, joints_num, sigma, from_rotations=False, offsets=None,
              return_rotations=False, fix_feet=False, blend=5, *, pin=None, pin_blend=5):
    """``joints_batch`` as a list per motion: joints (lens[i], J, 3), or with ``return_rotations`` (joints, rotations, offsets).
    ``pin`` / ``pin_blend``: limb pins as the last stage, as ``joints_batch`` takes them."""
    j, r, o, lens = joints_batch(motions, lens, dim_pose, mean, std, joints_num, sigma, from_rotations, offsets,
                                 return_rotations, fix_feet, blend, **pin_kw(pin, pin_blend))
    if return_rotations:
        return [(j[i, :n], r[i, :n], o[i]) for i, n in enumerate(lens)]
    return [j[i, :n] for i, n in enumerate(lens)]


def to_bvh(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, paths, fps, fps_out, euler, scale, target_rig=None,
           target_joint_map=None, target_up="Y", leg_ik=None, *, pin=None, pin_blend=5):
    """Rows -> one BVH text per motion: ``joints_batch`` with rotations and no filter, one
    ``motion_rig.rotations_to_rig`` over the padded batch, ``motion_rig.bvh_text`` per sample.  ``target_rig`` (BVH text, a
    path, a parsed file or ``motion_rig.target_rig``'s namespace; ``target_joint_map`` / ``target_up`` as it takes them): the
    motion goes onto that character's hierarchy instead, ``motion_rig.retarget_to_rig`` with ``leg_ik`` and
    ``motion_rig.target_bvh_text``; its units decide, so ``scale`` is refused.  ``pin`` / ``pin_blend``: limb pins (DESIGN.md
    §28) after ``fix_feet`` and before the export, as ``joints_batch`` takes them; the rotations turn with the limbs."""
    if target_rig is not None:
        if float(scale) != 1.0:
            raise ValueError("scale does not combine with target_rig: the target's own units decide")
        if not hasattr(target_rig, "table"):
            target_rig = make_target_rig(target_rig, target_joint_map, target_up, skeleton=skeleton_for_feats(dim_pose))
    j, r, o, lens = joints_batch(motions, lens, dim_pose, mean, std, (dim_pose + 1) // 12, 0.0, True, offsets, True,
                                 fix_feet=fix_feet, blend=blend, **pin_kw(pin, pin_blend))
    skel = skeleton_for_feats(dim_pose)
    rig = rig_of(skel)
    if target_rig is None:
        chan, lens_out = rotations_to_rig(j[:, :max(lens)], r[:, :max(lens)], torch.tensor(lens), skeleton=skel, euler=euler,
                                          fps=fps, fps_out=fps_out, scale=scale)
    else:
        chan, lens_out = retarget_to_rig(j[:, :max(lens)], r[:, :max(lens)], torch.tensor(lens), target_rig, offsets=o,
                                         skeleton=skel, euler=euler, fps=fps, fps_out=fps_out, leg_ik=leg_ik)
    num, den, fps = retime_ratio(skel, fps, fps_out)
    frame_time = den / (num * float(fps))
    chan, texts = chan.cpu(), []
    for i in range(len(lens)):
        if target_rig is None:
            texts.append(bvh_text(rig, o[i], chan[i], int(lens_out[i]), frame_time, euler=euler, scale=scale))
        else:
            texts.append(target_bvh_text(target_rig, chan[i], int(lens_out[i]), frame_time, euler=euler))
        if paths is not None and paths[i] is not None:
            with open(paths[i], "w") as f:
                f.write(texts[-1])
    return texts


def skinned_batch(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, mesh, pin, pin_blend):
    """What ``to_meshes`` and ``to_glb`` share: ``joints_batch`` as ``to_bvh`` runs it (forward kinematics, rotations, no
    filter, ``fix_feet``, pins), so that joints, rotations and pins agree, and the mesh: the caller's, or ``capsule_body`` of
    the offsets used, one body per motion.  -> (joints, rotations, offsets, lens, skeleton name, mesh)."""
    j, r, o, lens = joints_batch(motions, lens, dim_pose, mean, std, (dim_pose + 1) // 12, 0.0, True, offsets, True,
                                 fix_feet=fix_feet, blend=blend, **pin_kw(pin, pin_blend))
    skel = skeleton_for_feats(dim_pose)
    if mesh is None:
        mesh = capsule_body(o, skel)
    return j, r, o, lens, skel, mesh


def to_meshes(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, mesh=None, normals=False, *, pin=None, pin_blend=5):
    """Rows -> per motion ``(vertices (lens[i], V, 3), faces)``, with ``normals`` ``(vertices, normals, faces)`` (DESIGN.md
    §30): ``skinned_batch`` and one ``motion_mesh.skin_vertices`` over the padded batch.  ``faces`` (F, 3) is one tensor that
    every motion shares."""
    j, r, o, lens, skel, mesh = skinned_batch(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, mesh, pin, pin_blend)
    out = skin_vertices(mesh, j[:, :max(lens)], r[:, :max(lens)], torch.tensor(lens), return_normals=normals)
    faces = torch.from_numpy(mesh.faces)
    if normals:
        return [(out[0][i, :n], out[1][i, :n], faces) for i, n in enumerate(lens)]
    return [(out[i, :n], faces) for i, n in enumerate(lens)]


def to_glb(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, paths, fps, fps_out, scale, mesh=None, *, pin=None,
           pin_blend=5):
    """Rows -> one glTF binary per motion: ``skinned_batch``, one ``motion_rig.rotations_to_rig`` over the
    padded batch for the retimed root path and local quaternions, ``motion_mesh.glb_bytes`` per sample, written to
    ``paths[i]`` where given."""
    j, r, o, lens, skel, mesh = skinned_batch(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, mesh, pin, pin_blend)
    rig = rig_of(skel)
    chan, lens_out, quat = rotations_to_rig(j[:, :max(lens)], r[:, :max(lens)], torch.tensor(lens), skeleton=skel, fps=fps,
                                            fps_out=fps_out, return_quaternions=True)
    num, den, fps = retime_ratio(skel, fps, fps_out)
    frame_time = den / (num * float(fps))
    root, quat, o, out = chan[:, :, :3].cpu(), quat.cpu(), o.cpu(), []
    for i in range(len(lens)):
        out.append(glb_bytes(mesh.sample(i), rig, o[i], root[i], quat[i], int(lens_out[i]), frame_time, scale))
        if paths is not None and paths[i] is not None:
            with open(paths[i], "wb") as f:
                f.write(out[-1])
    return out


def to_frames(joints, size, camera, palette, style):
    """``motion_render.render_motion`` over a list of (n_i, J, 3) joint clips, one launch for all: a list of
    ``(n_i, H, W, 3)`` uint8 frames, or ``(n_i, H, W)`` palette indices."""
    x, lens = pad_clips(joints, joints[0].shape[1])
    frames = render_motion(x, lens, size=size, camera=camera, palette=palette, **(style or {}))
    return [frames[i, :n] for i, n in enumerate(lens.tolist())]


def to_world_frames(worlds, scene, tracks, size, camera, palette, style):
    """``motion_render.render_world`` over a list of worlds, each a list of (n_i, J, 3) joint clips in world
    coordinates, one call for all: per world ``(n, H, W, 3)`` uint8 frames or ``(n, H, W)`` palette indices, n the length of
    its longest character.  ``scene`` / ``tracks``: as ``render_world`` takes them; packed canvas-order track records
    (total, Km, REC), as ``generate_long`` takes them, are cut at the worlds' lengths."""
    lens = [max(int(c.shape[0]) for c in w) for w in worlds]
    if torch.is_tensor(tracks) and tracks.dim() == 3 and tracks.shape[0] == sum(lens) and len(lens) > 1:
        rows = torch.zeros((len(lens), max(lens)) + tuple(tracks.shape[1:]), dtype=tracks.dtype)
        for i, (n, part) in enumerate(zip(lens, torch.split(tracks.detach().cpu(), lens))):
            rows[i, :n] = part
        tracks = rows
    frames = render_world(worlds, scene=scene, tracks=tracks, size=size, camera=camera, palette=palette, **(style or {}))
    return [frames[i, :n] for i, n in enumerate(lens)]


def world_scene(characters):
    """The primitives a world is drawn with: the union of its characters' ``scene`` lists, in order, each primitive once."""
    out = []
    for c in characters:
        for p in c.get("scene") or []:
            if p not in out:
                out.append(p)
    return out


def to_frames_view(view, joints, cond, size, camera, palette, style):
    """``to_frames`` (``view`` "root", §21) or the world view of the same clips (``view`` "world", §26), one character to a
    world, with the ``scene`` / ``scene_tracks`` of ``cond`` that steered them."""
    if view == "root":
        return to_frames(joints, size, camera, palette, style)
    if view != "world":
        raise ValueError(f"view must be \"root\" or \"world\", not {view!r}")
    return to_world_frames([[j] for j in joints], cond.get("scene"), cond.get("scene_tracks"), size, camera, palette, style)


def to_body_frames(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, mesh, size, camera, palette, style, *, pin=None,
                   pin_blend=5):
    """Rows -> the body view, per motion ``(lens[i], H, W, 3)`` uint8 frames or ``(lens[i], H, W)`` palette
    indices: ``skinned_batch`` and ``motion_mesh.skin_vertices`` with normals, as ``to_meshes`` runs them, so that the body in
    the picture is the body in the ``.glb``, and one ``motion_render.render_mesh`` over the padded batch with the joints of
    the forward kinematics as root."""
    j, r, o, lens, skel, mesh = skinned_batch(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, mesh, pin, pin_blend)
    j, r = j[:, :max(lens)], r[:, :max(lens)]
    v, n = skin_vertices(mesh, j, r, torch.tensor(lens), return_normals=True)
    frames = render_mesh(v, mesh.faces, lens, root=j, normals=n, size=size, camera=camera, palette=palette, **(style or {}))
    return [frames[i, :k] for i, k in enumerate(lens)]


def to_gifs(frames, dim_pose, paths, fps):
    """One GIF per clip of palette frames: bytes, or ``paths[i]`` where given and written; ``fps`` defaults by ``dim_pose``."""
    if fps is None:
        fps = DEFAULT_FPS.get(skeleton_for_feats(dim_pose), DEFAULT_FPS["t2m"])
    if paths is None:
        return [gif_bytes(f, fps) for f in frames]
    return [gif_bytes(f, fps) if p is None else write_gif(f, p, fps) for f, p in zip(frames, paths)]
