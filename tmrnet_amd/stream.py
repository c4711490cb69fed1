"""Online per-frame phase recognition over live frame streams.

TMRNet is an online method: the prediction for frame f uses the clip ending at f and the
long-term feature bank (LFB) rows of earlier clips.  The reference only scores offline
(eval/python/test_singlenet_phase_non-local_pretrained_2fc_copy_mutiConv6_3.py:380-492: the bank
of the whole split first, then every clip); this module keeps what that loop needs per stream on
the device and answers every pushed frame:

* a ring of gate rows per stream and model -- ``trunk(frame) W_ih^T + b_ih + b_hh``, the per-frame
  part of the LSTM (as ``lfb_build.LFBBuilder.encode``), so a frame is encoded once by each model;
* a ring of bank rows per stream -- row s is the last hidden state of ``model_lfb`` over frames
  s .. s+T-1, causal because it ends at frame s+T-1;
* host row tables into both rings (``StreamState``), uploaded from pinned memory.

Per tick the two T-step recurrences read their sliding window of the gate ring in place
(``tmr_lstm_window_fwd``, window="kernel") or through a gather and per-step launches
(``LFBBuilder.recur``, window="steps"); the head is ``resnet_lstm.clip_head`` on bank rows
(``LFBRows``).  The outputs are those of ``evaluate.evaluate_split`` on a split consisting of that
one video with the bank ``lfb_build.build_lfb`` makes for it.
"""
import contextlib

import numpy as np
import torch

from . import health, ops
from .frames import RESIZE, margin_boxes, resize_frames
from .lfb_build import LFBBuilder, center_offset, check_activations, inference_mode
from .nlblock import LFBRows

WINDOWS = ("auto", "kernel", "steps")
# what window="auto" means: "kernel" beat "steps" by 14-17% of a tick at one stream in both
# geometries, spreads under 1.5% (scripts/stream_bench.py)
AUTO_WINDOW = "kernel"


class StreamState:
    """Host side of the rings: ages and row tables, no device.

    Frame number a of stream i (a = its age before the push) has gate-ring row
    ``i * Tcap + a % Tcap``; the clip starting at frame s has bank-ring row ``i * C + s % C``.
    Tcap >= T keeps the T frames of the newest clip; C >= L + 1 keeps the row written this tick
    next to the L rows before it, so no slot read at start s holds another start."""

    def __init__(self, seq_len, lfb_length, streams=1, gate_cap=None, bank_cap=None):
        T, L, S = int(seq_len), int(lfb_length), int(streams)
        if T < 1:
            raise ValueError("seq_len must be at least 1, got %d" % T)
        if L < 1:
            raise ValueError("lfb_length must be at least 1, got %d" % L)
        if S < 1:
            raise ValueError("streams must be at least 1, got %d" % S)
        self.T, self.L, self.S = T, L, S
        self.Tcap = T if gate_cap is None else int(gate_cap)
        self.C = L + 1 if bank_cap is None else int(bank_cap)
        if self.Tcap < T:
            raise ValueError("gate ring of %d rows cannot hold a clip of %d frames" % (self.Tcap, T))
        if self.C < L + 1:
            raise ValueError("bank ring of %d rows cannot hold %d rows and the new one"
                             % (self.C, L))
        self.ages = np.zeros(S, dtype=np.int64)

    def ids(self, streams=None):
        """The pushed stream ids as an int64 array (None: every stream, in order)."""
        if streams is None:
            return np.arange(self.S, dtype=np.int64)
        ids = np.atleast_1d(np.asarray(streams, dtype=np.int64))
        if ids.ndim != 1 or ids.size == 0:
            raise ValueError("streams must be a non-empty list of stream ids")
        if ids.min() < 0 or ids.max() >= self.S:
            raise ValueError("unknown stream id in %s: this recognizer has streams 0..%d"
                             % (ids.tolist(), self.S - 1))
        if np.unique(ids).size != ids.size:
            raise ValueError("a push carries one frame per stream; %s repeats one" % ids.tolist())
        return ids

    def gate_slots(self, ids):
        """Gate-ring row the frame pushed now goes to, per stream."""
        return ids * self.Tcap + self.ages[ids] % self.Tcap

    def ready(self, ids):
        """Streams whose push completes a clip (age + 1 >= T)."""
        return self.ages[ids] + 1 >= self.T

    def starts(self, ids):
        """Start frame of the clip the push completes (negative: not ready)."""
        return self.ages[ids] + 1 - self.T

    def window_rows(self, ids, starts):
        """(n, T) gate-ring rows of the clips starting at `starts`."""
        f = np.asarray(starts, dtype=np.int64)[:, None] + np.arange(self.T, dtype=np.int64)[None, :]
        return np.asarray(ids, dtype=np.int64)[:, None] * self.Tcap + f % self.Tcap

    def bank_slots(self, ids, starts):
        """Bank-ring row of the clips starting at `starts`."""
        return np.asarray(ids, dtype=np.int64) * self.C + np.asarray(starts, dtype=np.int64) % self.C

    def bank_rows(self, ids, starts):
        """(n, L) bank-ring rows of Lt: lfb.lfb_row_table of a split that is this one video
        (valid start v is row v, own-row fallback at start 0 included), mapped into the ring."""
        s = np.asarray(starts, dtype=np.int64)[:, None]
        q = np.maximum(s - np.arange(self.L, dtype=np.int64)[None, :] - 1, 0)
        return np.asarray(ids, dtype=np.int64)[:, None] * self.C + q % self.C

    def advance(self, ids):
        self.ages[ids] += 1

    def reset(self, stream):
        self.ages[self.ids([stream])] = 0


def _stride_runs(rows):
    """Split row indices into maximal runs of constant positive stride -> [(first index, count,
    stride)], so one strided GEMM writes each run."""
    out, i, n = [], 0, len(rows)
    while i < n:
        j = i + 1
        d = int(rows[j] - rows[i]) if j < n else 1
        if d <= 0:
            out.append((i, 1, 1))
            i = j
            continue
        while j + 1 < n and rows[j + 1] - rows[j] == d:
            j += 1
        j = min(j + 1, n)
        out.append((i, j - i, d))
        i = j
    return out


class OnlineRecognizer:
    """Per-frame phase recognition over `streams` independent live videos.

    model: a ``resnet_lstm`` (any backbone, with or without TimeConv); model_lfb: the
    ``resnet_lstm_LFB`` that fills the bank; both of the same ``seq_len`` and on the same device.
    activations: "fp32", "bf16" or "bf16-resnest" (lfb_build.check_activations, for both models).
    window: "kernel" (tmr_lstm_window_fwd), "steps" (gather + LFBBuilder.recur) or "auto".
    gate_cap / bank_cap: ring sizes per stream (default T and lfb_length + 1).
    cut_margin: cut each frame's black margin before the resize, as the reference prepares its
    frames (frames.margin_boxes).  A stream's box is taken from the first frame it pushes at age
    0, after construction or ``reset``, and reused for every later frame of that stream: an
    endoscope's border does not move within a video.  Taking it reads 16 bytes per new stream to
    the host, the only host read ``push`` makes, and only on those ticks.  Frames that already
    are 250 x 250 are cropped and resized too.  ``margin_box(stream)`` returns the box.
    """

    def __init__(self, model, model_lfb, lfb_length, streams=1, activations="fp32",
                 window="auto", gate_cap=None, bank_cap=None, cut_margin=False):
        if window not in WINDOWS:
            raise ValueError("window must be one of %s, got %r" % (WINDOWS, window))
        if model.seq_len != model_lfb.seq_len:
            raise ValueError("model has seq_len %d, model_lfb %d: the bank rows would not be "
                             "those of the model's clips" % (model.seq_len, model_lfb.seq_len))
        self.state = StreamState(model.seq_len, lfb_length, streams, gate_cap, bank_cap)
        check_activations(model, activations)
        check_activations(model_lfb, activations)
        self.model, self.model_lfb = model, model_lfb
        self.activations = activations
        self.window = AUTO_WINDOW if window == "auto" else window
        dev = self.device = next(model.parameters()).device
        if next(model_lfb.parameters()).device != dev:
            raise ValueError("model and model_lfb live on different devices")
        st = self.state
        H = model.lstm.hidden_size
        self.H = H
        self.gates = torch.zeros((st.S * st.Tcap, 4 * H), device=dev)
        self.gates_lfb = torch.zeros((st.S * st.Tcap, 4 * H), device=dev)
        self.bank = torch.zeros((st.S * st.C, H), device=dev)
        self._steps = (LFBBuilder(model), LFBBuilder(model_lfb))
        self._off = None
        self._bias = None
        # row tables go up from pinned memory; two buffers, each reused only after its copy landed
        n = st.S * (st.T + st.L + 2)
        self._pin = [torch.zeros(n, dtype=torch.int32, pin_memory=dev.type == "cuda")
                     for _ in range(2)]
        self._pin_ev = [None, None]
        self._tick = 0
        self._hist = [[] for _ in range(st.S)]
        self.cut_margin = bool(cut_margin)
        self._boxes = np.zeros((st.S, 4), dtype=np.int32)   # per stream, valid from its age 1 on
        self.mark = None   # optional callable(name): called after each phase of a tick was
        #                    enqueued (scripts/stream_bench.py times the phases with it)

    # ------------------------------------------------------------------ host helpers
    def age(self, stream):
        return int(self.state.ages[self.state.ids([stream])[0]])

    def reset(self, stream):
        """The stream starts a new video: its age is 0 again.  The rings are left alone (a stale
        row is never read: every row a tick reads was written after the reset)."""
        self.state.reset(stream)

    def margin_box(self, stream):
        """[r0, r1, c0, c1] cut out of the stream's frames (cut_margin=True), taken from the first
        frame of its current video; None before that frame."""
        i = int(self.state.ids([stream])[0])
        if not self.cut_margin or self.state.ages[i] == 0:
            return None
        return self._boxes[i].tolist()

    def _cut(self, u8, ids):
        """Crop every frame by its stream's box and resize it; streams at age 0 get their box."""
        new = np.nonzero(self.state.ages[ids] == 0)[0]
        if new.size:
            first = u8 if new.size == ids.size else u8[torch.from_numpy(new).to(u8.device)]
            self._boxes[ids[new]] = margin_boxes(first).cpu().numpy()
        return resize_frames(u8, RESIZE, boxes=self._boxes[ids])

    def health(self):
        """Raise if a window recurrence gave up a grid barrier and was not recomputed."""
        if self.device.type == "cuda":
            health.check(sync=True, device=self.device)

    def history(self, stream):
        """The stream's predictions so far (int64 ndarray), one per completed clip in push order:
        the valid-start order ``evaluate.export_phase`` takes (videos separated by reset())."""
        i = int(self.state.ids([stream])[0])
        self.health()
        if not self._hist[i]:
            return np.zeros(0, np.int64)
        return torch.cat(self._hist[i]).cpu().numpy()

    def _upload(self, tables):
        """One pinned -> device copy of the int32 tables; returns their device views."""
        k = self._tick & 1
        self._tick += 1
        if self._pin_ev[k] is not None:
            self._pin_ev[k].synchronize()
        pin, o = self._pin[k], 0
        for t in tables:
            pin[o:o + t.size] = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32).reshape(-1))
            o += t.size
        devt = pin[:o].to(self.device, non_blocking=True)
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            self._pin_ev[k] = ev
        out, o = [], 0
        for t in tables:
            out.append(devt[o:o + t.size].view(t.shape))
            o += t.size
        return out

    def _params(self):
        if self._bias is None:
            self._bias = [ops.residual_mask(m.lstm.bias_ih_l0.detach().contiguous(),
                                            m.lstm.bias_hh_l0.detach().contiguous(), None)
                          for m in (self.model, self.model_lfb)]
            self._off = torch.full((1, 2), center_offset(RESIZE[0]), dtype=torch.int32,
                                   device=self.device)
        return self._bias

    def refresh_parameters(self):
        """Call after the models' LSTM biases changed (the summed bias is cached)."""
        self._bias = None

    def _mark(self, name):
        if self.mark is not None:
            self.mark(name)

    # ------------------------------------------------------------------ the tick
    def _recur(self, which, gates, win, out, out_rows):
        """h_{T-1} of the clips whose gate rows are win (n, T) -> out rows out_rows."""
        model = (self.model, self.model_lfb)[which]
        w_hh = model.lstm.weight_hh_l0.detach()
        if self.window == "kernel":
            _, ws = ops.lstm_window_fwd(gates, win, w_hh, out=out, out_rows=out_rows)
            health.note_lstm(ws)
            return
        n, T = win.shape
        gx = ops.lfb_gather(gates, win).view(n * T, gates.shape[1])
        tmp = out if out_rows is None else torch.empty((n, self.H), device=self.device)
        self._steps[which].recur(gx, np.arange(n, dtype=np.int64) * T, tmp)
        if out_rows is not None:
            out.index_copy_(0, out_rows.long(), tmp)

    @torch.no_grad()
    def push(self, frames_u8, streams=None):
        """One new frame for each listed stream (None: all, in order).

        frames_u8: (S', H, W, 3) uint8 in host or device memory, or a callable returning it (a
        decoder; called with the stream ids).  Frames of another size than 250 x 250 are resized
        (frames.resize_frames); with cut_margin every frame is cropped by its stream's box first.
        Returns a dict: ``streams`` (ids), ``ready`` (host bool array:
        the push completed a clip, age + 1 >= T) and the device tensors ``preds``, ``scores``,
        ``probs``, ``logits``, ``lfb_rows`` with one row per pushed stream, meaningful where
        ready.  Nothing is copied to the host (but a new stream's box with cut_margin)."""
        st = self.state
        ids = st.ids(streams)
        n = ids.size
        with contextlib.ExitStack() as stack:
            stack.enter_context(inference_mode(self.model, self.activations))
            stack.enter_context(inference_mode(self.model_lfb, self.activations))
            u8 = frames_u8(ids.tolist()) if callable(frames_u8) else frames_u8
            if u8.dim() != 4 or u8.shape[0] != n or u8.shape[3] != 3 or u8.dtype != torch.uint8:
                raise ValueError("push: %d stream(s) need uint8 frames (%d, H, W, 3), got %s %s"
                                 % (n, n, u8.dtype, tuple(u8.shape)))
            bias = self._params()
            u8 = u8.to(self.device, non_blocking=True).contiguous()
            if self.cut_margin:
                u8 = self._cut(u8, ids)
            elif tuple(u8.shape[1:3]) != tuple(RESIZE):
                u8 = resize_frames(u8, RESIZE)
            x4 = ops.crop_normalize(u8, self._off, n)
            self._mark("input")
            slots = st.gate_slots(ids)
            for which, (model, ring) in enumerate(((self.model, self.gates),
                                                   (self.model_lfb, self.gates_lfb))):
                feat = model.share.features_nhwc4(x4)
                self._mark("trunks")
                w_ih = model.lstm.weight_ih_l0.detach()
                for i0, cnt, d in _stride_runs(slots):
                    ops.gemm_nt(feat[i0:i0 + cnt], w_ih, bias=bias[which],
                                out=ring[int(slots[i0]):], M=cnt, ldc=d * ring.shape[1])
                self._mark("projection")
            ready = st.ready(ids)
            out = {"streams": ids, "ready": ready}
            if ready.any():
                out.update(self._answer(ids, ready))
            else:
                K = self.model.fc_c.out_features
                dev = self.device
                out.update(preds=torch.zeros(n, dtype=torch.int64, device=dev),
                           scores=torch.zeros(n, device=dev), probs=torch.zeros((n, K), device=dev),
                           logits=torch.zeros((n, K), device=dev),
                           lfb_rows=torch.zeros((n, self.H), device=dev))
        st.advance(ids)
        for k in np.nonzero(ready)[0]:
            h = self._hist[int(ids[k])]
            h.append(out["preds"][k:k + 1])
            if len(h) >= 512:                 # one tensor per 512 ticks, not one per tick
                h[:] = [torch.cat(h)]
        return out

    def _answer(self, ids, ready):
        st = self.state
        rid = ids[ready]
        starts = st.starts(rid)
        nr, n = rid.size, ids.size
        where = np.nonzero(ready)[0]
        win, slot, lt, where_d = self._upload([st.window_rows(rid, starts),
                                               st.bank_slots(rid, starts),
                                               st.bank_rows(rid, starts), where])
        H = self.H
        self._recur(1, self.gates_lfb, win, self.bank, slot)          # bank row s, in place
        query = torch.empty((nr, H), device=self.device)
        self._recur(0, self.gates, win, query, None)
        self._mark("recurrences")
        logits = self.model.clip_head(query.view(nr, 1, H), LFBRows(self.bank, lt)).contiguous()
        probs, scores, preds = ops.softmax_max(logits)
        rows = ops.lfb_gather(self.bank, slot)
        self._mark("head")
        res = {"preds": preds, "scores": scores, "probs": probs, "logits": logits,
               "lfb_rows": rows}
        if nr == n:
            return res
        idx = where_d.long()
        full = {}
        for k, v in res.items():
            t = torch.zeros((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            full[k] = t.index_copy_(0, idx, v)
        return full
