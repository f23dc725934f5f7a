"""CPU: the fp64 evaluator restatement against the reference's outputs (tests/golden/evaluator.npz), our modules' state-dict
layout, the word vectorizer, the host FID step and the evaluator entry points' argument checks (no GPU needed)."""
import ctypes as C
import json
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg
import evaluator_ref as ER


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "evaluator.npz"))
    return g, json.loads(str(g["meta"]))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("tag", ["a", "a2", "b"])
def test_restatement_matches_reference_outputs(golden, tag):
    g, meta = golden
    case = meta["cases"][tag]
    state = ER.synth_state(case["dims"], case["seed"])
    w, p, x = ER.synth_inputs(case["B"], case["T"], case["dims"], case["seed"])
    t, m, mv = ER.co_embeddings(state, w, p, torch.tensor(case["cap_lens"]), x, torch.tensor(case["m_lens"]))
    assert _rel(t, g[f"{tag}_text"]) <= 1e-6
    assert _rel(m, g[f"{tag}_motion"]) <= 1e-6
    if f"{tag}_movements" in g:
        assert _rel(mv, g[f"{tag}_movements"]) <= 1e-6


def test_restatement_metrics_match_reference(golden):
    g, meta = golden
    c = meta["metrics"]
    s = c["seed"]
    t = ER.synth_embeddings((c["n_pairs"], 512), "text", s).numpy()
    m = (ER.synth_embeddings((c["n_pairs"], 512), "motion", s, 0.6) + torch.from_numpy(t) * 0.5).numpy()
    score, counts, size = ER.matching(t, m, c["batch_size"])
    assert size == int(g["c_r_size"]) and (counts == g["c_r_counts"]).all()
    assert abs(score / float(g["c_matching_score"]) - 1) <= 1e-6
    mu1, s1 = ER.stats(ER.synth_embeddings((c["n_gt"], 512), "gt", s).numpy())
    mu2, s2 = ER.stats(ER.synth_embeddings((c["n_gen"], 512), "gen", s, 0.8, 0.05).numpy())
    assert abs(ER.fid(mu1, s1, mu2, s2) / float(g["c_fid"]) - 1) <= 1e-6
    div = ER.diversity(ER.synth_embeddings((c["n_div"], 512), "div", s).numpy(), c["div_times"], c["div_seed"])
    assert abs(div / float(g["c_diversity"]) - 1) <= 1e-6
    mm = ER.multimodality(ER.synth_embeddings(tuple(c["mm"]) + (512,), "mm", s).numpy(), c["mm_times"], c["mm_seed"])
    assert abs(mm / float(g["c_multimodality"]) - 1) <= 1e-6


def test_state_dict_layout_matches_reference(golden):
    _, meta = golden
    E = pkg("evaluator")
    ev = E.MotionTextEvaluator()
    for name, want in meta["layout"].items():
        got = [[k, list(v.shape)] for k, v in getattr(ev, name).state_dict().items()]
        assert got == want, name
    # the restatement's synthetic weights use the same layout
    for name, keys in ER.state_layout().items():
        assert [[k, list(s)] for k, s, _ in keys] == meta["layout"][name]


def test_kit_widths_and_strict_load():
    E = pkg("evaluator")
    ev = E.MotionTextEvaluator(dim_pose=251)
    assert ev.movement_encoder.main[0].weight.shape == (512, 247, 4)
    st = ER.synth_state(dict(dim_pose=251), 0)
    ev.movement_encoder.load_state_dict(st["movement_encoder"], strict=True)
    ev.text_encoder.load_state_dict(st["text_encoder"], strict=True)
    ev.motion_encoder.load_state_dict(st["motion_encoder"], strict=True)


def _glove_dir(tmp_path):
    words = ["unk", "sos", "eos", "walk", "forward", "the", "person", "slowly", "arm"]
    vecs = np.arange(len(words) * 4, dtype=np.float32).reshape(len(words), 4)
    np.save(tmp_path / "our_vab_data.npy", vecs)
    with open(tmp_path / "our_vab_words.pkl", "wb") as f:
        pickle.dump(words, f)
    with open(tmp_path / "our_vab_idx.pkl", "wb") as f:
        pickle.dump({w: i for i, w in enumerate(words)}, f)
    return words, vecs


def test_word_vectorizer_crop_pad_vip_unknown(tmp_path):
    W = pkg("wordvec")
    words, vecs = _glove_dir(tmp_path)
    wv = W.WordVectorizer(str(tmp_path))
    assert len(wv) == len(words)
    short = ["the/DET", "person/NOUN", "walk/VERB", "forward/ADV", "slowly/ADV", "zebra/NOUN", "arm/NOUN", "the/XYZ"]
    long = ["walk/VERB"] * 25
    we, po, cl = wv.encode([short, long], max_text_len=20)
    assert we.shape == (2, 22, 4) and po.shape == (2, 22, 15) and we.dtype == np.float32
    assert cl.tolist() == [len(short) + 2, 22]
    idx = {w: i for i, w in enumerate(words)}
    oh = lambda p: W.POS_INDEX[p]  # noqa: E731
    # sos ... eos, then unk/OTHER padding
    assert (we[0, 0] == vecs[idx["sos"]]).all() and po[0, 0].argmax() == oh("OTHER")
    assert (we[0, len(short) + 1] == vecs[idx["eos"]]).all()
    assert all((we[0, k] == vecs[idx["unk"]]).all() and po[0, k].argmax() == oh("OTHER") for k in range(len(short) + 2, 22))
    # VIP overrides: walk -> Act_VIP, forward -> Loc_VIP, slowly -> Desc_VIP, arm -> Body_VIP; plain words keep their tag
    assert po[0, 1].argmax() == oh("DET") and po[0, 2].argmax() == oh("NOUN")
    assert po[0, 3].argmax() == oh("Act_VIP") and po[0, 4].argmax() == oh("Loc_VIP") and po[0, 5].argmax() == oh("Desc_VIP")
    assert po[0, 7].argmax() == oh("Body_VIP")
    # an unknown word: the unk vector and OTHER; an unknown tag: OTHER
    assert (we[0, 6] == vecs[idx["unk"]]).all() and po[0, 6].argmax() == oh("OTHER")
    assert po[0, 8].argmax() == oh("OTHER")
    assert np.all(po.sum(-1) == 1)
    # cropped: sos + the first 20 words + eos, no padding
    assert (we[1, 1:21] == vecs[idx["walk"]]).all() and (we[1, 21] == vecs[idx["eos"]]).all()


def test_host_fid_equals_scipy_sqrtm():
    scipy_linalg = pytest.importorskip("scipy.linalg")
    M = pkg("eval_metrics")
    rng = np.random.RandomState(0)
    D = 64
    a, b = rng.randn(300, D), rng.randn(280, D) @ rng.randn(D, D) * 0.3 + 0.1
    mu1, s1 = a.mean(0), np.cov(a, rowvar=False)
    mu2, s2 = b.mean(0), np.cov(b, rowvar=False)
    covmean = scipy_linalg.sqrtm(s1 @ s2).real
    diff = mu1 - mu2
    want = diff @ diff + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean)
    got = M.frechet_distance(mu1, s1, mu2, s2)
    assert abs(got / want - 1) <= 1e-9, (got, want)


def test_metric_statistics():
    M = pkg("eval_metrics")
    v = np.array([[1.0, 2.0], [3.0, 2.0], [2.0, 5.0]])
    mean, ci = M.metric_statistics(v)
    assert np.allclose(mean, v.mean(0)) and np.allclose(ci, 1.96 * v.std(0) / np.sqrt(3))


def test_evaluator_abi_argument_validation_without_gpu():
    L = pkg("_lib")
    lib = L.lib()
    ARG, UNS = 1, 3
    lens = (C.c_int32 * 2)(3, 5)
    zero = (C.c_int32 * 2)(0, 5)
    long_ = (C.c_int32 * 2)(3, 9)
    p = C.c_void_p(256)  # never dereferenced: every case below is refused before any launch
    ws = lib.mdm_gru_bidir_workspace_bytes(2, 32)
    assert ws == 2 * 2 * 2 * 32 * 4
    assert lib.mdm_gru_bidir_workspace_bytes(0, 32) == -1

    def gru(gx=p, lens_host=lens, H=32, T=8, wsb=ws):
        return lib.mdm_gru_bidir(gx, p, p, p, p, lens_host, 2, T, H, p, p, C.c_int64(wsb), None)

    assert gru(gx=None) == ARG
    assert gru(lens_host=None) == ARG
    assert gru(lens_host=zero) == ARG        # len = 0
    assert gru(lens_host=long_) == ARG       # len > T
    assert gru(wsb=ws - 4) == ARG            # short workspace
    assert gru(H=40) == UNS                  # H % 16 != 0
    assert gru(H=2048) == UNS                # H > 1024
    assert lib.mdm_eval_pad_rows(None, C.c_int64(4), 1, 4, 4, 8, 1, 0, p, None) == ARG
    assert lib.mdm_eval_pad_rows(p, C.c_int64(4), 1, 4, 4, 2, 1, 0, p, None) == ARG  # Cp < C
    assert lib.mdm_eval_pad_rows(p, C.c_int64(4), 1, 4, 4, 4, 1, 0, p, None) == ARG  # re-layout in place
    assert lib.mdm_eval_ln_leaky(None, 1, 4, p, p, C.c_float(1e-5), p, None) == ARG
    assert lib.mdm_eval_matching(None, p, 4, 8, None, p, p, None) == ARG
    assert lib.mdm_eval_matching(p, p, 4, 8, None, None, p, None) == ARG
    assert lib.mdm_eval_matching(p, p, 16000, 512, None, p, p, None) == UNS
    assert lib.mdm_eval_center(p, 0, 8, p, p, None) == ARG


def test_evaluator_rejects_bad_lengths_before_the_device():
    E = pkg("evaluator")
    with pytest.raises(Exception):
        E._check_lens(np.array([0, 3]), 8, "lengths")
    with pytest.raises(Exception):
        E._check_lens(np.array([9, 3]), 8, "lengths")
    E._check_lens(np.array([1, 8]), 8, "lengths")
    assert E.MotionTextEvaluator.align_index(torch.tensor([5, 9, 5, 2])).tolist() == \
        np.argsort([5, 9, 5, 2])[::-1].tolist()
