"""The device entropy decoder's host side and logic without a GPU: tmr_jpeg_scan_pack
(tmrnet_amd/csrc/jpeg_host.cpp) against a Python unstuffing of each fixture's scan, and the
decode scheme of jpeg_entropy.hip -- the shared core tmrnet_amd/csrc/jpeg_entropy.h, run serially
by the stand-alone driver tests/jpeg_entropy_main.cpp -- against the host decoder on every fixture
of tests/golden/jpeg_cases.npz at sub_bits 64, 256 and the default; then the same driver under the
host sanitizers on the fixtures, on every prefix and on single-byte corruptions of one of them.
The driver is a program of its own: nothing is loaded into this process but the library."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _jpeg_emu as emu
from tests.test_jpeg_cpu import MUTATED, _sanitizer_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = emu.load_cases()
OK = [c for c in CASES if c[1] == "ok"]
RST = [c for c in OK if c[0].endswith("_rst3") or c[0].endswith("_rstrow")]
PACKED = [c for c in OK if c not in RST]


def cut_scan(data):
    """`data` without the last tenth of its scan but with its end marker: the probe accepts it,
    both entropy decoders run out of bits.  tests/test_jpeg_entropy_gpu.py sends the kernel this
    input after the drivers below have run it."""
    assert data.endswith(b"\xff\xd9")
    cut = data[:len(data) * 9 // 10]
    return (cut[:-1] if cut.endswith(b"\xff") else cut) + b"\xff\xd9"


CUT = ("cut_noise_70x50_420_q75", "cut", (50, 70), "",
       cut_scan(next(c[4] for c in OK if c[0] == "noise_70x50_420_q75")))


def _pack(data, bits_cap=None, tables_cap=None, bits_off=0, tables_off=0):
    """(status, info, desc, bits, tables) of tmr_jpeg_scan_pack; the buffers are pre-filled with
    0xA5 so that what a refused call wrote would show."""
    from tmrnet_amd import _lib
    cap = (len(data) + 8 + 15) // 16 * 16 if bits_cap is None else bits_cap
    tcap = _lib.JPEG_MAX_TABLES * ctypes.sizeof(_lib.JpegHuff) if tables_cap is None else tables_cap
    bits = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    tables = np.full(max(tcap, 1), 0xA5, dtype=np.uint8)
    info, desc = _lib.JpegInfo(), _lib.JpegScanDesc()
    rc = _lib.lib().tmr_jpeg_scan_pack(data, len(data), ctypes.byref(info), bits.ctypes.data, cap,
                                       bits_off, tables.ctypes.data, tcap, tables_off,
                                       ctypes.byref(desc))
    return rc, info, desc, bits, tables


def _scan_offset(data):
    """First byte after the SOS segment, by a marker walk of its own."""
    pos = 2
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        seg = (data[pos] << 8) | data[pos + 1]
        pos += seg
        if m == 0xDA:
            return pos


def _unstuff(data):
    out, pos = bytearray(), _scan_offset(data)
    while pos < len(data):
        b = data[pos]
        if b == 0xFF:
            if pos + 1 < len(data) and data[pos + 1] == 0:
                pos += 1
            else:
                break
        out.append(b)
        pos += 1
    return bytes(out)


def test_fixture_counts():
    assert len(OK) == 77 and len(RST) == 11 and len(PACKED) == 66


@pytest.mark.parametrize("case", PACKED, ids=[c[0] for c in PACKED])
def test_pack_equals_python_unstuffing(case):
    from tmrnet_amd import _lib, jpeg
    name, _, (h, w), _, data = case
    rc, info, d, bits, tables = _pack(data, bits_off=4096, tables_off=160)
    assert rc == 0, _lib.lib().tmr_last_error()
    want = _unstuff(data)
    assert d.nbits == 8 * len(want)
    assert d.bits_bytes == (len(want) + 8 + 15) // 16 * 16 <= bits.size
    assert bits[:len(want)].tobytes() == want
    assert not bits[len(want):d.bits_bytes].any()             # the padding is zero
    assert (bits[d.bits_bytes:] == 0xA5).all()                # and nothing past it is touched
    p = jpeg.probe(data)
    assert (d.width, d.height, d.ncomp) == (p.width, p.height, p.ncomp) == (w, h, p.ncomp)
    assert jpeg.SAMPLING[d.sampling] == p.sampling
    assert tuple(d.blocks_w) == p.blocks_w and tuple(d.blocks_h) == p.blocks_h
    assert tuple(info.blocks_w) == p.blocks_w and int(info.coef_bytes) == p.coef_bytes
    assert (d.bits_off, d.tables_off) == (4096, 160)
    lum = 4 if p.sampling == "4:2:0" else 1
    assert d.mcu_blocks == lum + p.ncomp - 1
    assert list(d.slot_comp)[:d.mcu_blocks] == [0] * lum + list(range(1, p.ncomp))
    assert 1 <= d.ntables <= _lib.JPEG_MAX_TABLES
    assert all(t < d.ntables for t in list(d.dc_table)[:p.ncomp] + list(d.ac_table)[:p.ncomp])
    used = d.ntables * ctypes.sizeof(_lib.JpegHuff)
    assert (tables[used:] == 0xA5).all()
    t0 = _lib.JpegHuff.from_buffer_copy(tables[:ctypes.sizeof(_lib.JpegHuff)].tobytes())
    assert 0 < t0.nsym <= 256 and any(t0.lut)


def test_pack_status_codes():
    from tmrnet_amd import _lib
    for name, kind, _, _, data in CASES:
        rc = _pack(data)[0]
        if kind == "malformed":
            assert rc == 1, name
        elif kind == "unsupported":
            assert rc == 2, name
    for name, _, _, _, data in RST:
        rc = _pack(data)[0]
        assert rc == _lib.JPEG_HOST_PASS == 4, name
        assert b"restart" in _lib.lib().tmr_last_error()


def test_pack_refuses_small_buffers_before_writing():
    from tmrnet_amd import _lib
    data = next(c[4] for c in OK if c[0] == "noise_70x50_420_q75")
    rc, _, d, _, _ = _pack(data)
    assert rc == 0
    rc, _, _, bits, tables = _pack(data, bits_cap=d.bits_bytes - 16)
    assert rc == 3 and b"bit buffer too small" in _lib.lib().tmr_last_error()
    assert (bits == 0xA5).all() and (tables == 0xA5).all()
    rc, _, _, bits, tables = _pack(data, tables_cap=d.ntables * ctypes.sizeof(_lib.JpegHuff) - 1)
    assert rc == 3 and b"table buffer too small" in _lib.lib().tmr_last_error()
    assert (bits == 0xA5).all() and (tables == 0xA5).all()
    assert _pack(data, bits_cap=d.bits_bytes)[0] == 0          # the exact size is enough
    assert _pack(data, bits_off=8)[0] == 3


def test_ws_query_refuses_bad_arguments():
    from tmrnet_amd import _lib
    assert _lib.query("tmr_jpeg_entropy_ws_bytes", 2, 4096, 0) == 16 + 2 * 4 * 20
    assert _lib.query("tmr_jpeg_entropy_ws_bytes", 1, 0, 64) == 16 + 20
    for f, sub in ((0, 0), (1, 32), (1, 100), (1, -64)):
        with pytest.raises(RuntimeError, match="tmr_jpeg_entropy_ws_bytes"):
            _lib.query("tmr_jpeg_entropy_ws_bytes", f, 4096, sub)


def _host_compiler():
    """A host C++ compiler: $CXX, the system's, or the one the library itself is built with."""
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cxx and shutil.which(cxx):
            return [cxx]
    return [os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc", "-x", "c++"]


def _build(tmp, argv, name):
    exe = os.path.join(tmp, name)
    subprocess.check_call(argv + ["-I" + os.path.join(ROOT, "include"),
                                  os.path.join(ROOT, "tests", "jpeg_entropy_main.cpp"),
                                  os.path.join(ROOT, "tmrnet_amd", "csrc", "jpeg_host.cpp"), "-o", exe])
    return exe


def _write(tmp, cases):
    paths = []
    for name, _, _, _, data in cases:
        p = os.path.join(tmp, name + ".bin")
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    return paths


def _counts(stdout):
    m = re.match(r"inputs (\d+): device ok (\d+), device refused (\d+), host pass (\d+), "
                 r"not packed (\d+), max rounds (\d+)\n$", stdout)
    assert m, stdout
    return [int(v) for v in m.groups()]


def test_serial_scheme_equals_host_decoder_on_every_fixture(tmp_path):
    """The plain build: the driver compares the scheme's coefficients with
    tmr_jpeg_entropy_decode's at sub_bits 64, 256 and the default, and exits 1 on a difference."""
    tmp = str(tmp_path)
    exe = _build(tmp, _host_compiler() + ["-std=c++17", "-O2"], "jpeg_entropy_main")
    r = subprocess.run([exe, "1", "0"] + _write(tmp, PACKED + [CUT]), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    inputs, ok, refused, host_pass, not_packed, rounds = _counts(r.stdout)
    assert (inputs, ok, refused, host_pass, not_packed) == (67, 66, 1, 0, 0)   # refused: CUT
    assert rounds >= 2   # at 64 bits a fixture needs more than one round: the rounds are exercised


def test_scheme_under_host_sanitizers(tmp_path):
    tmp = str(tmp_path)
    argv, reason = _sanitizer_compiler(tmp)
    if argv is None:
        pytest.skip(reason)
    exe = _build(tmp, argv, "jpeg_entropy_main_san")
    paths = _write(tmp, sorted(CASES, key=lambda c: c[0] != MUTATED) + [CUT])
    assert os.path.basename(paths[0]) == MUTATED + ".bin"
    nbytes = os.path.getsize(paths[0])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "12345", "1"] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    inputs, ok, refused, host_pass, not_packed, _ = _counts(r.stdout)
    assert inputs == len(CASES) + 1 + 4 * nbytes
    assert ok >= 66 and host_pass >= 11 and not_packed >= 6
    assert refused > 0   # corruptions inside the scan reached the error recovery
