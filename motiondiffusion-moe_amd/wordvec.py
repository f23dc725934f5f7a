"""GloVe word vectors + part-of-speech one-hots for the evaluator's text encoder, from a LOCAL directory holding the
reference's files ``<prefix>_data.npy``, ``<prefix>_words.pkl`` and ``<prefix>_idx.pkl`` (utils/word_vectorizer.py).
Host numpy only: the result is what ``MotionTextEvaluator.get_co_embeddings`` takes as ``word_embs`` / ``pos_ohot``."""
from __future__ import annotations

import os
import pickle
from typing import List, Sequence

import numpy as np

POS_TAGS = ("VERB", "NOUN", "DET", "ADP", "NUM", "AUX", "PRON", "ADJ", "ADV", "Loc_VIP", "Body_VIP", "Obj_VIP", "Act_VIP",
            "Desc_VIP", "OTHER")
POS_INDEX = {p: i for i, p in enumerate(POS_TAGS)}

# words whose part of speech the vectorizer overrides with a "VIP" class (first class that lists the word wins)
_VIP = (
    ("Loc_VIP", "left right clockwise counterclockwise anticlockwise forward back backward up down straight curve"),
    ("Body_VIP", "arm chin foot feet face hand mouth leg waist eye knee shoulder thigh"),
    ("Obj_VIP", "stair dumbbell chair window floor car ball handrail baseball basketball"),
    ("Act_VIP", "walk run swing pick bring kick put squat throw hop dance jump turn stumble stop sit lift lower raise wash "
                "stand kneel stroll rub bend balance flap jog shuffle lean rotate spin spread climb"),
    ("Desc_VIP", "slowly carefully fast careful slow quickly happy angry sad happily angrily sadly"),
)
VIP_POS = {}
for _cls, _words in _VIP:
    for _w in _words.split():
        VIP_POS.setdefault(_w, _cls)


class WordVectorizer:
    def __init__(self, meta_root: str, prefix: str = "our_vab"):
        vectors = np.load(os.path.join(meta_root, f"{prefix}_data.npy"))
        with open(os.path.join(meta_root, f"{prefix}_words.pkl"), "rb") as f:
            words = pickle.load(f)
        with open(os.path.join(meta_root, f"{prefix}_idx.pkl"), "rb") as f:
            word2idx = pickle.load(f)
        self.word2vec = {w: vectors[word2idx[w]] for w in words}
        self.dim_word = int(vectors.shape[1])

    def __len__(self):
        return len(self.word2vec)

    @staticmethod
    def pos_onehot(pos: str) -> np.ndarray:
        v = np.zeros(len(POS_TAGS))
        v[POS_INDEX.get(pos, POS_INDEX["OTHER"])] = 1
        return v

    def __getitem__(self, item: str):
        """``"word/POS"`` -> (word vector, POS one-hot); unknown words map to ``unk`` / OTHER."""
        word, pos = item.split("/")
        if word in self.word2vec:
            return self.word2vec[word], self.pos_onehot(VIP_POS.get(word, pos))
        return self.word2vec["unk"], self.pos_onehot("OTHER")

    def encode(self, tokens_list: Sequence[Sequence[str]], max_text_len: int = 20):
        """Token lists (``"word/POS"``) -> (word_embs (B, max_text_len + 2, dim_word) float32,
        pos_ohot (B, max_text_len + 2, 15) float32, cap_lens (B,) int64), as Text2MotionDatasetV2.__getitem__
        (datasets1/evaluator.py:262-279): ``sos`` / ``eos`` around the caption, cropped to ``max_text_len`` words, padded
        with ``unk/OTHER``."""
        W, P, lens = [], [], []
        for tokens in tokens_list:
            tokens = list(tokens)
            if len(tokens) < max_text_len:
                tokens = ["sos/OTHER"] + tokens + ["eos/OTHER"]
                n = len(tokens)
                tokens = tokens + ["unk/OTHER"] * (max_text_len + 2 - n)
            else:
                tokens = ["sos/OTHER"] + tokens[:max_text_len] + ["eos/OTHER"]
                n = len(tokens)
            pairs: List = [self[t] for t in tokens]
            W.append(np.stack([p[0] for p in pairs]))
            P.append(np.stack([p[1] for p in pairs]))
            lens.append(n)
        return (np.stack(W).astype(np.float32), np.stack(P).astype(np.float32), np.asarray(lens, dtype=np.int64))
