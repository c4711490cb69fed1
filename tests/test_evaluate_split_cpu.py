"""Host-side rules of the single-pass split evaluation (tmrnet_amd/evaluate.SplitEvaluator): the
clip -> label rule, merge_results and the argument errors.  No GPU."""
import numpy as np
import pytest
import torch

import tmrnet_amd
from tmrnet_amd import evaluate, lfb_build
from tmrnet_amd.lfb import LongFeatureBank, get_useful_start_idx
from tmrnet_amd.sampler import SeqSampler


@pytest.mark.parametrize("T,lengths", [(3, [6, 2, 5]), (10, [25, 9, 10, 31]), (1, [4, 3])])
def test_clip_label_rule(T, lengths):
    """Literal restatement of the reference: the test split's index list is every valid start
    followed by its T-1 successors, read in order by SeqSampler; the labels of the loaded frames
    are sliced labels[(T-1)::T] (:455)."""
    n = sum(lengths)
    labels = np.random.default_rng(0).integers(0, 7, n)
    starts = get_useful_start_idx(T, lengths)
    idx = []
    for s in starts:
        for j in range(T):
            idx.append(s + j)
    loaded = np.array([labels[i] for i in SeqSampler(None, idx)])
    want = loaded[(T - 1)::T]
    got = labels[evaluate.clip_label_index(T, lengths)]
    assert got.tolist() == want.tolist() and len(got) == len(starts)


def _shard(n, k=7, seed=0, frames=0):
    g = np.random.default_rng(seed)
    probs = g.random((n, k)).astype(np.float32)
    preds = probs.argmax(1).astype(np.int64) if n else np.zeros(0, np.int64)
    labels = g.integers(0, k, n).astype(np.int64)
    loss = float(g.random()) * n
    return evaluate._finish({
        "preds": preds, "scores": probs.max(1) if n else np.zeros(0, np.float32),
        "labels": labels, "probs": probs, "logits": np.log(probs + 1e-3),
        "loss_sum": loss, "logit_loss_sum": 2 * loss, "corrects": int((preds == labels).sum()),
        "frames_encoded": frames, "clips": n})


def test_merge_results():
    parts = [_shard(4, seed=1, frames=6), _shard(0, frames=0), _shard(3, seed=2, frames=5)]
    m = evaluate.merge_results(parts)
    assert m["preds"].tolist() == parts[0]["preds"].tolist() + parts[2]["preds"].tolist()
    assert m["probs"].shape == (7, 7) and m["logits"].shape == (7, 7) and m["scores"].shape == (7,)
    assert m["labels"].tolist() == parts[0]["labels"].tolist() + parts[2]["labels"].tolist()
    assert m["loss_sum"] == pytest.approx(parts[0]["loss_sum"] + parts[2]["loss_sum"])
    assert m["logit_loss_sum"] == pytest.approx(2 * m["loss_sum"])
    assert m["clips"] == 7 and m["frames_encoded"] == 11
    assert m["corrects"] == parts[0]["corrects"] + parts[2]["corrects"]
    assert m["accuracy"] == pytest.approx(m["corrects"] / 7)
    assert m["average_loss"] == pytest.approx(m["loss_sum"] / 7)
    empty = evaluate.merge_results([_shard(0)])
    assert empty["clips"] == 0 and empty["accuracy"] == 0.0 and empty["average_loss"] == 0.0
    with pytest.raises(ValueError):
        evaluate.merge_results([])


def test_argument_errors():
    T, lengths = 3, [6, 2, 5]
    m = tmrnet_amd.resnet_lstm(seq_len=T)
    valid = get_useful_start_idx(T, lengths)
    frames = torch.zeros(13, 250, 250, 3, dtype=torch.uint8)
    labels = torch.zeros(13, dtype=torch.int64)
    bank = LongFeatureBank(torch.zeros(len(valid), 512), valid, 5, "cpu")
    with pytest.raises(ValueError, match="labels cover 12 frames"):
        evaluate.evaluate_split(m, bank, frames, lengths, labels[:12])
    other = get_useful_start_idx(T, [6, 3, 5])
    bad = LongFeatureBank(torch.zeros(len(other), 512), other, 5, "cpu")
    with pytest.raises(ValueError, match="valid starts"):
        evaluate.evaluate_split(m, bad, frames, lengths, labels)
    with pytest.raises(ValueError, match="precision='bf16'"):
        evaluate.evaluate_split(m, bank, frames, lengths, labels, activations="bf16")
    with pytest.raises(ValueError, match="activations must be"):
        evaluate.evaluate_split(m, bank, frames, lengths, labels, activations="fp16")
    with pytest.raises(ValueError, match="precision='bf16'"):
        lfb_build.LFBBuilder(tmrnet_amd.resnet_lstm_LFB(seq_len=T), activations="bf16")
    assert m.training and m.share.infer_act16 is False   # nothing was switched on the way
