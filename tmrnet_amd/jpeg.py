"""Baseline JPEG frames decoded on the device after a host entropy pass: an opt-in replacement for
the PIL decode of ``tmrnet_amd.frames`` that returns the same bytes as ``pil_loader``
(train_only_non-local_pretrained.py:96-99).

The host does the serial part of each file -- marker parse and Huffman decode into DCT
coefficients (``tmr_jpeg_entropy_decode``, jpeg_host.cpp; C++ called through ctypes, which drops
the GIL, so plain threads scale) -- straight into one of two pinned buffers.  One asynchronous copy
takes a batch's coefficients and quantisation tables to HBM, where ``tmr_jpeg_reconstruct``
(jpeg.hip) dequantises, runs the 8x8 inverse DCT, upsamples the chroma and converts to packed RGB:
(F, H, W, 3) uint8, the input of ``frames.resize_frames``.

Files outside the decoder's scope (progressive, 4:2:2, CMYK, PNG, ...: ``probe`` status 2) are
decoded by ``pil_loader`` into their place in the batch, so a batch may mix both kinds and every
frame still equals ``pil_loader``'s; a malformed file (status 1) raises.

``DeviceJpegDecoder(entropy="device")`` (opt-in) moves the Huffman decode to the device as well:
the host only parses the headers and packs each scan (``tmr_jpeg_scan_pack``: the entropy-coded
bytes without their stuffing, the file's Huffman tables, a descriptor), the upload is the
compressed scan, and ``tmr_jpeg_entropy_decode_device`` (jpeg_entropy.hip) writes the coefficients
in device memory.  Files with a restart interval keep the host entropy pass inside the same batch.
On this route ``result()`` reads one status word per frame back -- one small copy and one stream
synchronise per batch, which the default route does not have; a frame with a non-zero status goes
through the host entropy pass, which raises with its message.
"""
import ctypes
import io
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from . import _lib
from ._lib import call, query, stream_ptr
from .frames import pil_loader

MAX_WORKERS = 16   # a fixed cap: the host share of one GPU, never the machine's CPU count
SAMPLING = {0: "gray", 1: "4:4:4", 2: "4:2:0"}

JpegProbe = namedtuple("JpegProbe", "status reason width height ncomp sampling blocks_w blocks_h "
                                    "coef_bytes")


def _probe(data):
    info = _lib.JpegInfo()
    rc = _lib.lib().tmr_jpeg_probe(data, len(data), ctypes.byref(info))
    reason = _lib.lib().tmr_last_error().decode() if rc else ""
    return rc, reason, info


def probe(data):
    """What the headers of `data` (the bytes of a file) say: status 0 = a baseline JPEG the device
    decodes, 1 = malformed or truncated, 2 = well formed but out of scope (left to PIL), with the
    reason; the sizes are meaningful for status 0 only."""
    rc, reason, i = _probe(bytes(data))
    return JpegProbe(rc, reason, i.width, i.height, i.ncomp, SAMPLING.get(i.sampling) if rc == 0 else None,
                     tuple(i.blocks_w), tuple(i.blocks_h), int(i.coef_bytes))


def _align(n, a=16):
    return (n + a - 1) // a * a


_DESC = ctypes.sizeof(_lib.JpegScanDesc)
_TABLES = _lib.JPEG_MAX_TABLES * ctypes.sizeof(_lib.JpegHuff)


class _Frame:
    __slots__ = ("name", "data", "info", "rgb", "shape", "dev")


class JpegJob:
    """A batch whose host pass is running (``DeviceJpegDecoder.submit``); ``result()`` waits for
    it, then enqueues the copy and the kernels on the current stream."""

    def __init__(self, dec, slot, future):
        self._dec, self._slot, self._future, self._out = dec, slot, future, None

    def result(self):
        if self._out is None:
            try:
                plan = self._future.result()
                self._out = self._dec._device_pass(self._slot, plan)
            finally:
                self._dec._owner[self._slot] = None
        return self._out


class DeviceJpegDecoder:
    """``decode(items)`` -> (F, H, W, 3) uint8 on `device`, equal to ``pil_loader`` of each item
    (a path, or the bytes of a file).  ``submit(items)`` returns at once with a job whose
    ``result()`` gives the same tensor: the host pass of batch i + 1 overlaps the step on batch i.
    Two batches may be in flight (two pinned buffers); a buffer is not written again before the
    copy and the kernels that read it have finished.  ``stats`` counts the frames decoded on the
    device (``"device"``) and those that fell back to PIL (``"fallback"``), and of the former
    those whose entropy decode ran on the device (``"entropy_device"``) and on the host
    (``"entropy_host"``).  `entropy` = "host" (default) or "device" selects where the Huffman
    decode runs (module docstring); `sub_bits` is the device decoder's subsequence length
    (0: its default)."""

    def __init__(self, workers=16, device="cuda", entropy="host", sub_bits=0):
        if entropy not in ("host", "device"):
            raise RuntimeError("DeviceJpegDecoder: entropy must be 'host' or 'device', got %r" % (entropy,))
        sub_bits = int(sub_bits)
        if sub_bits != 0 and (sub_bits < 64 or sub_bits % 32):
            raise RuntimeError("DeviceJpegDecoder: sub_bits=%d is neither 0 nor a multiple of 32 >= 64"
                               % sub_bits)
        self.entropy, self.sub_bits = entropy, sub_bits
        self.workers = max(1, min(MAX_WORKERS, int(workers)))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceJpegDecoder: a cuda device is required, got %s" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.stats = {"device": 0, "fallback": 0, "entropy_device": 0, "entropy_host": 0}
        self.kernel_events = None    # a list: (start, end) events around each batch's kernels
        self.entropy_events = []     # with kernel_events: (start, end) around the entropy kernels
        self.entropy_rounds = []     # with kernel_events: re-decode rounds each frame needed
        self._pool = ThreadPoolExecutor(max_workers=self.workers)
        self._coord = ThreadPoolExecutor(max_workers=2)
        self._host = [None, None]    # pinned uint8 buffers
        self._busy = [None, None]    # event after the last device work that reads the buffer
        self._owner = [None, None]   # job whose host pass owns the buffer
        self._next = 0

    # ---- host pass (worker threads) ----
    @staticmethod
    def _load(item):
        fr = _Frame()
        fr.rgb = None
        fr.dev = False
        if isinstance(item, (bytes, bytearray, memoryview)):
            fr.name, fr.data = "<bytes>", bytes(item)
        else:
            fr.name = str(item)
            with open(item, "rb") as f:
                fr.data = f.read()
        rc, reason, fr.info = _probe(fr.data)
        if rc == 1:
            raise RuntimeError("tmr_jpeg_probe failed (1): %s: %s" % (fr.name, reason))
        if rc == 0:
            fr.shape = (fr.info.height, fr.info.width)
        else:   # out of scope: the reference's loader
            if isinstance(item, (bytes, bytearray, memoryview)):
                with Image.open(io.BytesIO(fr.data)) as img:
                    fr.rgb = np.asarray(img.convert("RGB"))
            else:
                fr.rgb = np.asarray(pil_loader(item))
            fr.info = None
            fr.shape = fr.rgb.shape[:2]
        return fr

    def _load_packable(self, item):
        """_load, and whether the device entropy decoder takes the file (no restart interval)."""
        fr = self._load(item)
        if fr.info is not None:
            rc = _lib.lib().tmr_jpeg_scan_pack(fr.data, len(fr.data), ctypes.byref(fr.info), None, 0, 0,
                                               None, 0, 0, None)
            if rc not in (0, _lib.JPEG_HOST_PASS):
                raise RuntimeError("tmr_jpeg_scan_pack failed (%d): %s: %s"
                                   % (rc, fr.name, _lib.lib().tmr_last_error().decode()))
            fr.dev = rc == 0
        return fr

    def _buffer(self, slot, nbytes):
        ev = self._busy[slot]
        if ev is not None:
            ev.synchronize()
            self._busy[slot] = None
        buf = self._host[slot]
        if buf is None or buf.numel() < nbytes:
            buf = self._host[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return buf

    def _map(self, fn, seq):
        """[fn(x) for x in seq] on the worker threads, a few chunks per thread: the executor's
        per-task cost (taken under the GIL) is paid per chunk, not per frame.  Returns, or raises
        the first chunk's exception, only when every chunk has ended: none is left writing into
        the pinned buffer after the batch has given it up."""
        n = len(seq)
        step = max(1, -(-n // (4 * self.workers)))
        futures = [self._pool.submit(lambda lo=lo: [fn(x) for x in seq[lo:lo + step]])
                   for lo in range(0, n, step)]
        failed = False
        for f in futures:
            if failed and f.cancel():   # not started yet: never will
                continue
            failed = f.exception() is not None or failed   # waits for the chunk to end
        return [y for f in futures if not f.cancelled() for y in f.result()]

    def _host_pass(self, slot, items):
        frames = self._map(self._load if self.entropy == "host" else self._load_packable, items)
        h, w = frames[0].shape
        for fr in frames:
            if fr.shape != (h, w):
                raise RuntimeError("DeviceJpegDecoder: %s is %s, expected %s" % (fr.name, fr.shape, (h, w)))
        # one buffer: per sampling class its frames' coefficients (host entropy pass) or packed
        # scans (device entropy pass: descriptors, Huffman tables, bits), quantisation tables and
        # output indices; then the fallback frames' RGB and indices
        groups, at = [], 0
        classes = sorted({(fr.info.sampling, not fr.dev) for fr in frames if fr.info is not None})
        for s, on_host in classes:
            idx = [i for i, fr in enumerate(frames)
                   if fr.info is not None and fr.info.sampling == s and fr.dev != on_host]
            cb = int(frames[idx[0]].info.coef_bytes)
            g = {"sampling": s, "idx": idx, "coef_bytes": cb, "entropy": "host" if on_host else "device"}
            if on_host:
                g["coef"] = at
                at += cb * len(idx)
            else:
                g["desc"] = at
                at += _DESC * len(idx)
                g["tables"] = at
                at += _TABLES * len(idx)
                g["bits"] = []
                for i in idx:
                    g["bits"].append(at)
                    at += _align(len(frames[i].data) + 8)
            g["qt"] = at
            at += 384 * len(idx)
            g["index"] = at
            at = _align(at + 4 * len(idx))
            groups.append(g)
        fb = [i for i, fr in enumerate(frames) if fr.info is None]
        plan = {"n": len(frames), "h": h, "w": w, "groups": groups, "fb": fb, "fb_rgb": at}
        at = _align(at + len(fb) * h * w * 3)
        plan["fb_index"] = at
        at = _align(at + 8 * len(fb))
        plan["bytes"] = at
        host = self._buffer(slot, max(at, 16))
        arr = host.numpy()
        base = host.data_ptr()
        fn = _lib.lib().tmr_jpeg_entropy_decode
        last_error = _lib.lib().tmr_last_error

        pack = _lib.lib().tmr_jpeg_scan_pack

        def decode_one(job):
            g, j, i = job
            fr = frames[i]
            if g["entropy"] == "device":
                o, t = g["bits"][j], g["tables"] + j * _TABLES
                rc = pack(fr.data, len(fr.data), ctypes.byref(fr.info), base + o,
                          _align(len(fr.data) + 8), o, base + t, _TABLES, t, base + g["desc"] + j * _DESC)
                if rc != 0:
                    raise RuntimeError("tmr_jpeg_scan_pack failed (%d): %s: %s"
                                       % (rc, fr.name, last_error().decode()))
                q = g["qt"] + 384 * j
                arr[q:q + 384] = np.frombuffer(fr.info.qt, dtype=np.uint8)
                return
            rc = fn(fr.data, len(fr.data), ctypes.byref(fr.info), base + g["coef"] + j * g["coef_bytes"],
                    g["coef_bytes"])
            if rc != 0:
                raise RuntimeError("tmr_jpeg_entropy_decode failed (%d): %s: %s"
                                   % (rc, fr.name, last_error().decode()))
            q = g["qt"] + 384 * j
            arr[q:q + 384] = np.frombuffer(fr.info.qt, dtype=np.uint8)

        jobs = []
        for g in groups:
            o = g["index"]
            arr[o:o + 4 * len(g["idx"])] = np.asarray(g["idx"], dtype=np.int32).view(np.uint8)
            jobs += [(g, j, i) for j, i in enumerate(g["idx"])]
        self._map(decode_one, jobs)
        for g in groups:
            if g["entropy"] == "device":   # word 4 of a descriptor: its bit count
                d = arr[g["desc"]:g["desc"] + _DESC * len(g["idx"])].view(np.uint32)
                g["max_bits"] = int(d.reshape(len(g["idx"]), _DESC // 4)[:, 4].max())
        plan["frames"] = frames
        for j, i in enumerate(fb):
            o = plan["fb_rgb"] + j * h * w * 3
            arr[o:o + h * w * 3] = frames[i].rgb.reshape(-1)
        o = plan["fb_index"]
        arr[o:o + 8 * len(fb)] = np.asarray(fb, dtype=np.int64).view(np.uint8)
        return plan

    # ---- device pass (caller's thread, current stream) ----
    def _device_pass(self, slot, plan):
        n, h, w = plan["n"], plan["h"], plan["w"]
        with torch.cuda.device(self.device):
            dbuf = torch.empty(plan["bytes"], dtype=torch.uint8, device=self.device)
            dbuf.copy_(self._host[slot][:plan["bytes"]], non_blocking=True)
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
            base = dbuf.data_ptr()
            if self.kernel_events is not None:
                timed = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                timed[0].record(torch.cuda.current_stream(self.device))
            # the entropy kernels of every device group first, then the reconstruction
            dev_groups = [g for g in plan["groups"] if g["entropy"] == "device"]
            status = rounds = None
            if dev_groups:
                status = torch.empty(sum(len(g["idx"]) for g in dev_groups), dtype=torch.int32,
                                     device=self.device)
                rounds, so = [], 0
                for g in dev_groups:
                    f = len(g["idx"])
                    g["coef_dev"] = torch.empty(f * g["coef_bytes"], dtype=torch.uint8, device=self.device)
                    nb = query("tmr_jpeg_entropy_ws_bytes", f, g["max_bits"], self.sub_bits)
                    ews = torch.empty(nb, dtype=torch.uint8, device=self.device)
                    call("tmr_jpeg_entropy_decode_device", ctypes.c_void_p(base + g["desc"]), dbuf,
                         ctypes.c_size_t(plan["bytes"]), f, h, w, g["sampling"], g["max_bits"],
                         self.sub_bits, g["coef_dev"], status[so:so + f], ews, ctypes.c_size_t(nb),
                         stream_ptr(self.device))
                    rounds.append(ews[:4 * f].view(torch.int32))
                    so += f
                if self.kernel_events is not None:
                    mid = torch.cuda.Event(enable_timing=True)
                    mid.record(torch.cuda.current_stream(self.device))
                    self.entropy_events.append((timed[0], mid))
            for g in plan["groups"]:
                f = len(g["idx"])
                nb = query("tmr_jpeg_ws_bytes", f, h, w, g["sampling"])
                ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
                coef = g.pop("coef_dev") if g["entropy"] == "device" else ctypes.c_void_p(base + g["coef"])
                call("tmr_jpeg_reconstruct", coef,
                     ctypes.c_void_p(base + g["qt"]), f, h, w, g["sampling"], ws,
                     ctypes.c_size_t(nb), out, ctypes.c_void_p(base + g["index"]), n,
                     stream_ptr(self.device))
            fb = plan["fb"]
            if fb:
                rgb = dbuf[plan["fb_rgb"]:plan["fb_rgb"] + len(fb) * h * w * 3].view(len(fb), h, w, 3)
                index = dbuf[plan["fb_index"]:plan["fb_index"] + 8 * len(fb)].view(torch.int64)
                out.index_copy_(0, index, rgb)
            if self.kernel_events is not None:
                timed[1].record(torch.cuda.current_stream(self.device))
                self.kernel_events.append(timed)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._busy[slot] = ev
            if dev_groups:
                self._check_status(plan, dev_groups, status.cpu())   # the route's one synchronise
                if self.kernel_events is not None:
                    self.entropy_rounds += torch.cat(rounds).cpu().tolist()
        on_device = sum(len(g["idx"]) for g in dev_groups)
        self.stats["entropy_device"] += on_device
        self.stats["entropy_host"] += n - len(fb) - on_device
        self.stats["device"] += n - len(fb)
        self.stats["fallback"] += len(fb)
        return out

    @staticmethod
    def _check_status(plan, dev_groups, status):
        """A frame the device entropy decoder refused goes through the host's, which refuses the
        same scans and says why; a scan only one of them refuses is a bug in one of them."""
        if not bool(status.any()):
            return
        order = [i for g in dev_groups for i in g["idx"]]
        for i, st in zip(order, status.tolist()):
            if st == 0:
                continue
            fr = plan["frames"][i]
            coef = np.empty(int(fr.info.coef_bytes) // 2, dtype=np.int16)
            rc = _lib.lib().tmr_jpeg_entropy_decode(fr.data, len(fr.data), ctypes.byref(fr.info),
                                                    coef.ctypes.data, coef.nbytes)
            if rc != 0:
                raise RuntimeError("tmr_jpeg_entropy_decode failed (%d): %s: %s"
                                   % (rc, fr.name, _lib.lib().tmr_last_error().decode()))
            raise RuntimeError("DeviceJpegDecoder: the device entropy decoder refused %s (status %d) "
                               "but the host decoder accepts it: a bug, not a fallback" % (fr.name, st))

    def submit(self, items):
        items = list(items)
        if not items:
            raise RuntimeError("DeviceJpegDecoder: no frames")
        if self._pool is None:
            raise RuntimeError("DeviceJpegDecoder: closed")
        slot = self._next
        if self._owner[slot] is not None:
            raise RuntimeError("DeviceJpegDecoder: two batches are in flight already; take the "
                               "result() of the older one first")
        self._next = 1 - slot
        job = JpegJob(self, slot, self._coord.submit(self._host_pass, slot, items))
        self._owner[slot] = job
        return job

    def decode(self, items):
        return self.submit(items).result()

    def host_pass(self, items):
        """The host pass alone, for measurement: files read and entropy-decoded (or, with
        entropy="device", packed) into a pinned buffer, nothing copied or launched.  Returns the
        bytes a batch uploads."""
        job = self.submit(items)
        try:
            return job._future.result()["bytes"]
        finally:
            self._owner[job._slot] = None

    def close(self):
        if self._pool is not None:
            self._coord.shutdown(wait=True)
            self._pool.shutdown(wait=True)
            self._pool = self._coord = None
        for s in range(2):
            if self._busy[s] is not None:
                self._busy[s].synchronize()
                self._busy[s] = None
            self._host[s] = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
