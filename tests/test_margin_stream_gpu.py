"""OnlineRecognizer(cut_margin=True): a stream fed bordered frames answers with the bits of a
plain stream fed the same frames cropped by the first frame's box and resized on the host
(Pillow), the box is taken again after reset(), and the flag off changes nothing."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import _margin_emu as emu
from tests.test_stream_gpu import L, SEED, T, make_pair, stream_video
from tmrnet_amd.stream import OnlineRecognizer

pytestmark = pytest.mark.gpu

N = 5
SHAPE = (120, 214)


def bordered_video(seed, n=N):
    """n frames of one video: the same disc (the border does not move), new texture and salt."""
    h, w = SHAPE
    first = emu.disc_frame(h, w, seed)
    rng = np.random.default_rng(1000 + seed)
    out = [first]
    for _ in range(n - 1):
        f = first.copy()
        lit = f.any(axis=2)
        f[lit] = rng.integers(60, 256, size=(int(lit.sum()), 3), dtype=np.uint8)
        out.append(f)
    return np.stack(out)


def host_cut(video, box):
    r0, r1, c0, c1 = box
    return torch.from_numpy(np.stack([
        np.asarray(Image.fromarray(f, "RGB").crop((c0, r0, c1, r1)).resize((250, 250), Image.BILINEAR))
        for f in video]))


@pytest.fixture(scope="module")
def pair(dev):
    c = make_pair(SEED, n=1)
    c["model"].to(dev).eval()
    c["model_lfb"].to(dev).eval()
    return c


def test_cut_margin_stream(pair, dev):
    video = bordered_video(0)
    box = emu.box(video[0])
    assert box != [0, SHAPE[0], 0, SHAPE[1]]
    rec = OnlineRecognizer(pair["model"], pair["model_lfb"], L, window="kernel", cut_margin=True)
    assert rec.margin_box(0) is None
    ready, a = stream_video(rec, torch.from_numpy(video))
    assert ready == [False] * (T - 1) + [True] * (N - T + 1)
    assert rec.margin_box(0) == box
    plain = OnlineRecognizer(pair["model"], pair["model_lfb"], L, window="kernel")
    _, b = stream_video(plain, host_cut(video, box))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert plain.margin_box(0) is None

    # a new video after reset(): another border, so another box; frames already 250 x 250
    rec.reset(0)
    assert rec.margin_box(0) is None
    big = np.zeros((T, 250, 250, 3), np.uint8)
    rng = np.random.default_rng(7)
    big[:, 30:200, 40:230] = rng.integers(60, 256, size=(T, 170, 190, 3), dtype=np.uint8)
    box2 = emu.box(big[0])
    assert box2 == [30, 199, 40, 229]
    _, a2 = stream_video(rec, torch.from_numpy(big))
    assert rec.margin_box(0) == box2
    plain.reset(0)
    _, b2 = stream_video(plain, host_cut(big, box2))
    assert a2["logits"].shape[0] == 1
    for k in a2:
        assert torch.equal(a2[k], b2[k]), k


def test_two_streams_keep_their_own_boxes(pair, dev):
    """Streams that start on different ticks: each takes its box on its own first frame."""
    v0, v1 = bordered_video(1, n=T + 1), bordered_video(2, n=T)
    assert emu.box(v0[0]) != emu.box(v1[0])
    rec = OnlineRecognizer(pair["model"], pair["model_lfb"], L, streams=2, window="kernel",
                           cut_margin=True)
    plain = OnlineRecognizer(pair["model"], pair["model_lfb"], L, streams=2, window="kernel")
    c0, c1 = host_cut(v0, emu.box(v0[0])), host_cut(v1, emu.box(v1[0]))
    rec.push(torch.from_numpy(v0[:1]), streams=[0])
    plain.push(c0[:1], streams=[0])
    answers = 0
    for i in range(T):
        a = rec.push(torch.from_numpy(np.stack([v1[i], v0[i + 1]])), streams=[1, 0])
        b = plain.push(torch.stack([c1[i], c0[i + 1]]), streams=[1, 0])
        assert a["ready"].tolist() == b["ready"].tolist()
        answers += int(a["ready"].sum())
        assert torch.equal(a["logits"], b["logits"]), i
    assert answers == 3
    assert rec.margin_box(0) == emu.box(v0[0]) and rec.margin_box(1) == emu.box(v1[0])


def test_flag_off_is_unchanged(pair, dev):
    video = torch.from_numpy(bordered_video(3))
    _, a = stream_video(OnlineRecognizer(pair["model"], pair["model_lfb"], L, window="kernel",
                                         cut_margin=False), video)
    _, b = stream_video(OnlineRecognizer(pair["model"], pair["model_lfb"], L, window="kernel"),
                        video)
    for k in a:
        assert torch.equal(a[k], b[k]), k
