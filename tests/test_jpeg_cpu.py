"""The host half of the JPEG decode (tmrnet_amd/csrc/jpeg_host.cpp) without a GPU: its
coefficients, put through the numpy emulation of the device half (tests/_jpeg_emu.py), give
Pillow's RGB decode bit for bit on every supported fixture of tests/golden/jpeg_cases.npz; the
probe sorts the other fixtures into out-of-scope (2) and malformed (1); threads decode side by
side; and a stand-alone driver runs the parser under the host sanitizers on the fixtures, on every
prefix and on single-byte corruptions of one of them."""
import ctypes
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _jpeg_emu as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = emu.load_cases()
OK = [c for c in CASES if c[1] == "ok"]
MUTATED = "smooth_17x17_420_q75"


def _decode(data):
    """(info, coefficients) of the host decoder; asserts status 0."""
    from tmrnet_amd import _lib, jpeg
    p = jpeg.probe(data)
    assert p.status == 0, p
    info = _lib.JpegInfo()
    coef = np.full(p.coef_bytes // 2, 0x5a5a, dtype=np.int16)   # every entry must be overwritten
    rc = _lib.lib().tmr_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data,
                                            coef.nbytes)
    assert rc == 0, _lib.lib().tmr_last_error()
    assert info.coef_bytes == p.coef_bytes
    return info, coef


def test_fixture_file_covers_the_listed_cases():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    assert len(OK) >= 69 and sum(c[1] == "unsupported" for c in CASES) == 4
    assert sum(c[1] == "malformed" for c in CASES) == 2
    assert os.path.getsize(emu.GOLDEN) < 1 << 20


@pytest.mark.parametrize("case", OK, ids=[c[0] for c in OK])
def test_host_coefficients_reconstruct_to_pillow(case):
    name, _, (h, w), sha, data = case
    info, coef = _decode(data)
    assert (info.height, info.width) == (h, w)
    rgb = emu.reconstruct(coef, h, w, info.sampling, list(info.blocks_h), list(info.blocks_w),
                          np.array(info.qt))
    assert emu.sha(rgb) == sha                      # the committed Pillow 12.2.0 decode
    assert np.array_equal(rgb, emu.pil_rgb(data))   # this machine's Pillow


def test_one_lookup_table_holds_eight_value_bits():
    """Hand-built files whose AC table gives the size-8 symbol a 1-bit code: code + value bits fill
    the 9-bit table exactly, with |value| up to 255 (value * 256 needs more than 16 bits)."""
    hand = [c for c in OK if c[0].startswith("hand_8x8_ac1_")]
    assert len(hand) == 4
    for name, _, _, _, data in hand:
        _, coef = _decode(data)
        want = np.zeros(64, dtype=np.int16)
        want[1] = int(name.rsplit("_", 1)[1])
        assert np.array_equal(coef, want), (name, coef[:4])


def test_probe_sizes_match_pillow():
    from PIL import Image
    import io
    from tmrnet_amd import jpeg
    for name, _, (h, w), _, data in OK:
        p = jpeg.probe(data)
        with Image.open(io.BytesIO(data)) as im:
            assert (p.width, p.height) == im.size == (w, h), name
            assert p.ncomp == (1 if im.mode == "L" else 3), name
        mcu = 16 if p.sampling == "4:2:0" else 8
        assert p.blocks_w[0] * 8 == -(-w // mcu) * mcu and p.blocks_h[0] * 8 == -(-h // mcu) * mcu
        assert p.coef_bytes == 128 * sum(a * b for a, b in zip(p.blocks_w, p.blocks_h))
    # 854x480 4:2:0: the coefficient upload next to the 1,229,760-byte RGB upload it replaces
    assert 128 * (108 * 60 + 2 * 54 * 30) == 1244160


def test_probe_reports_unsupported_and_malformed():
    from tmrnet_amd import jpeg
    want = {"progressive_37x29": "progressive", "422_37x29": "subsampling",
            "cmyk_37x29": "components", "png_37x29": "not a JPEG"}
    for name, kind, _, _, data in CASES:
        p = jpeg.probe(data)
        if kind == "unsupported":
            assert p.status == 2 and want[name] in p.reason, (name, p)
        elif kind == "malformed":
            assert p.status == 1 and p.reason, (name, p)


def test_truncated_scan_is_malformed_not_read_past():
    """A cut inside the entropy-coded data: the probe misses the end marker, the decoder runs out
    of bits; both say 1."""
    from tmrnet_amd import _lib, jpeg
    data = next(c[4] for c in OK if c[0] == "noise_70x50_420_q75")
    cut = data[:len(data) * 9 // 10]
    good = jpeg.probe(data)
    p = jpeg.probe(cut)
    assert p.status == 1 and "truncated" in p.reason
    info = _lib.JpegInfo()
    coef = np.zeros(good.coef_bytes // 2, dtype=np.int16)
    rc = _lib.lib().tmr_jpeg_entropy_decode(cut, len(cut), ctypes.byref(info), coef.ctypes.data,
                                            coef.nbytes)
    assert rc == 1 and b"truncated" in _lib.lib().tmr_last_error()
    # a buffer that is too small is refused before anything is written
    rc = _lib.lib().tmr_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data,
                                            coef.nbytes - 128)
    assert rc == 3 and b"too small" in _lib.lib().tmr_last_error()


def test_sixteen_threads_equal_serial():
    items = [c[4] for c in OK[:50]]
    assert len(items) == 50
    serial = [_decode(d)[1] for d in items]
    with ThreadPoolExecutor(max_workers=16) as ex:
        rounds = list(ex.map(lambda i: _decode(items[i % 50])[1], range(16 * 50)))
    for i, c in enumerate(rounds):
        assert np.array_equal(c, serial[i % 50]), i


def _sanitizer_compiler(tmp):
    """(argv prefix, None) of a host compiler that links a sanitized program with the runtime
    inside it, or (None, reason).  The runtime is linked statically so that the program does not
    depend on the order of the process's preloaded libraries."""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    tried = []
    for cxx, extra in ((os.environ.get("CXX"), []), ("g++", ["-static-libasan", "-static-libubsan"]),
                       ("clang++", ["-static-libsan"])):
        if not cxx or not shutil.which(cxx):
            continue
        if not extra:
            extra = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
        argv = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                "-fno-sanitize-recover=undefined"] + extra
        r = subprocess.run(argv + [probe, "-o", os.path.join(tmp, "probe")], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([os.path.join(tmp, "probe")]).returncode == 0:
            return argv, None
        tried.append("%s: %s" % (cxx, (r.stderr.strip().splitlines() or ["probe program failed"])[-1]))
    return None, "no host compiler links the address/undefined sanitizer runtime (%s)" % "; ".join(tried or ["none found"])


def test_parser_under_host_sanitizers(tmp_path):
    tmp = str(tmp_path)
    argv, reason = _sanitizer_compiler(tmp)
    if argv is None:
        pytest.skip(reason)
    exe = os.path.join(tmp, "jpeg_host_main")
    subprocess.check_call(argv + ["-I" + os.path.join(ROOT, "include"),
                                  os.path.join(ROOT, "tests", "jpeg_host_main.cpp"),
                                  os.path.join(ROOT, "tmrnet_amd", "csrc", "jpeg_host.cpp"), "-o", exe])
    paths = []
    for name, _, _, _, data in sorted(CASES, key=lambda c: c[0] != MUTATED):
        p = os.path.join(tmp, name + ".bin")
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    assert os.path.basename(paths[0]) == MUTATED + ".bin"
    # the parser allocates nothing; the leak checker needs ptrace, which sandboxes often deny
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "12345"] + paths, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("calls "), r.stdout
