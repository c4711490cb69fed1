"""Host rules of the online recognizer (tmrnet_amd/stream.py): the ring row tables against
lfb.lfb_row_table, the ready / reset state machine, the argument errors, and the host checks of
tmr_lstm_window_fwd.  No GPU."""
import numpy as np
import pytest
import torch

import tmrnet_amd
from tmrnet_amd import _lib, lfb
from tmrnet_amd.stream import OnlineRecognizer, StreamState, _stride_runs

T, L, C, N = 3, 5, 6, 11


def test_bank_table_is_the_single_video_row_table():
    """Every start of an 11-frame video: the ring table is lfb_row_table of a split that is this
    one video, mapped mod C, and every slot it reads holds the start asked for (the slot's last
    writer among starts 0..s)."""
    st = StreamState(T, L, streams=2, bank_cap=C)
    sid = np.array([1])
    valid = list(range(N - T + 1))
    holds = {}                                   # ring slot -> start written last
    for s in valid:
        holds[int(st.bank_slots(sid, [s])[0])] = s          # the tick writes its row first
        want = lfb.lfb_row_table(valid, [s], L)              # (1, L) valid-start rows = starts
        got = st.bank_rows(sid, [s])
        assert got.shape == (1, L)
        assert (got == 1 * C + want % C).all(), s
        for k in range(L):
            assert holds[int(got[0, k])] == int(want[0, k]), (s, k)
    assert lfb.lfb_row_table(valid, [0], L).tolist() == [[0] * L]   # own-row fallback


@pytest.mark.parametrize("tcap", [T, T + 3])
def test_window_rows_across_wrap(tcap):
    """The gate-ring rows of every clip hold that clip's frames, across wrap-around."""
    st = StreamState(T, L, streams=3, gate_cap=tcap)
    sid = np.array([2])
    holds = {}                                   # ring row -> frame written last
    for a in range(N):
        assert st.ages[2] == a
        row = int(st.gate_slots(sid)[0])
        assert row == 2 * tcap + a % tcap
        holds[row] = a
        if st.ready(sid)[0]:
            s = int(st.starts(sid)[0])
            assert s == a + 1 - T
            win = st.window_rows(sid, [s])
            assert win.shape == (1, T)
            assert [holds[int(r)] for r in win[0]] == list(range(s, s + T))
        st.advance(sid)


def test_ring_sizes_checked():
    with pytest.raises(ValueError, match="gate ring"):
        StreamState(T, L, gate_cap=T - 1)
    with pytest.raises(ValueError, match="bank ring"):
        StreamState(T, L, bank_cap=L)


def test_ready_mask_and_reset():
    """Two streams of different ages: stream 0 leads by two frames; reset starts over."""
    st = StreamState(T, L, streams=2)
    seen = []
    for ids in ([0], [0], [0, 1], [1, 0], [1], [0, 1]):
        ids = st.ids(ids)
        seen.append(st.ready(ids).tolist())
        st.advance(ids)
    assert seen == [[False], [False], [True, False], [False, True], [True], [True, True]]
    assert st.ages.tolist() == [5, 4]
    assert st.starts(st.ids(None)).tolist() == [3, 2]
    st.reset(1)
    assert st.ages.tolist() == [5, 0]
    assert st.ready(st.ids(None)).tolist() == [True, False]
    assert st.gate_slots(st.ids([1])).tolist() == [1 * T + 0]


def test_stride_runs():
    assert _stride_runs(np.array([4])) == [(0, 1, 1)]
    assert _stride_runs(np.array([1, 4, 7, 10])) == [(0, 4, 3)]
    assert _stride_runs(np.array([1, 4, 8, 12, 2])) == [(0, 2, 3), (2, 2, 4), (4, 1, 1)]
    assert _stride_runs(np.array([5, 2, 3])) == [(0, 1, 1), (1, 2, 1)]


def test_argument_errors():
    m = tmrnet_amd.resnet_lstm(seq_len=T)
    f = tmrnet_amd.resnet_lstm_LFB(seq_len=T)
    with pytest.raises(ValueError, match="seq_len"):
        OnlineRecognizer(m, tmrnet_amd.resnet_lstm_LFB(seq_len=T + 1), L)
    with pytest.raises(ValueError, match="lfb_length"):
        OnlineRecognizer(m, f, 0)
    with pytest.raises(ValueError, match="activations must be"):
        OnlineRecognizer(m, f, L, activations="fp16")
    with pytest.raises(ValueError, match="precision='bf16'"):
        OnlineRecognizer(m, f, L, activations="bf16")
    with pytest.raises(ValueError, match="window must be"):
        OnlineRecognizer(m, f, L, window="fused")
    rec = OnlineRecognizer(m, f, L, streams=2)
    assert rec.window == "kernel"                # what "auto" means
    frame = torch.zeros(1, 250, 250, 3, dtype=torch.uint8)
    for bad in ([2], [-1], [0, 0]):
        with pytest.raises(ValueError):
            rec.push(torch.zeros(len(bad), 250, 250, 3, dtype=torch.uint8), streams=bad)
    with pytest.raises(ValueError, match="unknown stream id"):
        rec.reset(2)
    with pytest.raises(ValueError, match="unknown stream id"):
        rec.age(5)
    with pytest.raises(ValueError, match="uint8 frames"):
        rec.push(frame, streams=[0, 1])          # one frame for two streams
    assert rec.age(0) == 0 and rec.age(1) == 0   # nothing was pushed on the way
    assert m.training and f.training and m.share.infer_act16 is False
    assert rec.history(1).size == 0


def test_window_entry_host_checks():
    with pytest.raises(RuntimeError, match="tmr_lstm_window_ws_bytes: bad sizes"):
        _lib.query("tmr_lstm_window_ws_bytes", -1, 3, 512)
    assert _lib.query("tmr_lstm_window_ws_bytes", 5, 10, 512) >= 256 + 5 * 10 * 512 * 4
    with pytest.raises(RuntimeError, match="tmr_lstm_window_fwd: bad sizes"):
        _lib.call("tmr_lstm_window_fwd", None, 0, None, 2, -3, 512, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match="tmr_lstm_window_fwd: null operand"):
        _lib.call("tmr_lstm_window_fwd", None, 0, None, 2, 3, 512, None, None, None, None, 0, None)
    one = torch.zeros(4)                         # any non-null host address: checked, never read
    with pytest.raises(RuntimeError, match="tmr_lstm_window_fwd: workspace"):
        _lib.call("tmr_lstm_window_fwd", one.data_ptr(), 4, one.data_ptr(), 2, 3, 512,
                  one.data_ptr(), one.data_ptr(), None, None, 0, None)
