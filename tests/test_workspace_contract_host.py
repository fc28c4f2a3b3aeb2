"""The harness of tests/workspace_contract.py against a fake library on the host: Python callables that write through the
pointers they are handed.  What the GPU cases rely on is shown here -- a byte written past the workspace, in front of it
or past an output is reported, a well-behaved call passes and gets its outputs back -- and the table of outputs is
complete: no compute entry point of include/statdepth_hip.h is outside it."""
import ctypes

import numpy as np
import pytest

from statdepth_amd import _native
from workspace_contract import (BACK_GUARD, CANARY, EXCLUDED, FRONT_GUARD, OUTPUTS, POISONS, ContractProxy, ContractViolation,
                                Guarded, Memory, compute_symbols, takes_stream, takes_workspace)


def _poke(address, value=0x11):
    ctypes.c_ubyte.from_address(address).value = value


def _bytes(address, count):
    return np.frombuffer((ctypes.c_ubyte * count).from_address(address), dtype=np.uint8).copy()


class FakeLib:
    """sd_mbd_counts(X, T, n, st, sn, targets, m, J, algo, out, ws, ws_bytes, stream) with m (J - 1) int64 of output:
    writes q + 1 to out[q], scribbles over its whole workspace, and one stray byte where `stray` says.  sd_l1_depth has no
    workspace.  Anything else is not there."""

    def __init__(self, stray=None):
        self.stray = stray
        self.seen = {}

    def sd_mbd_counts(self, X, T, n, st, sn, targets, m, J, algo, out, ws, ws_bytes, stream):
        self.seen = {"ws": ws, "ws_bytes": ws_bytes, "out": out,
                     "ws_in": _bytes(ws, ws_bytes) if ws else None, "out_in": _bytes(out, m * (J - 1) * 8)}
        count = m * (J - 1)
        np.frombuffer((ctypes.c_int64 * count).from_address(out), dtype=np.int64)[:] = np.arange(1, count + 1)
        if ws:
            ctypes.memset(ws, 0x77, ws_bytes)
        if self.stray == "past_ws":
            _poke(ws + ws_bytes)
        elif self.stray == "far_past_ws":
            _poke(ws + ws_bytes + BACK_GUARD - 1)
        elif self.stray == "before_ws":
            _poke(ws - 1)
        elif self.stray == "past_out":
            _poke(out + count * 8)
        elif self.stray == "before_out":
            _poke(out - 1)
        return 0

    def sd_l1_depth(self, P, n, d, targets, m, out, stream):
        np.frombuffer((ctypes.c_double * m).from_address(out), dtype=np.float64)[:] = 0.5
        return 0

    def sd_last_error(self):
        return b""


def _call(proxy, m=5, J=3, ws_bytes=1000, ws=True):
    out = np.full(m * (J - 1), -1, dtype=np.int64)
    caller_ws = np.full(max(ws_bytes, 1), 0x33, dtype=np.uint8)
    rc = proxy.sd_mbd_counts(0, 7, 9, 9, 1, None, m, J, 0, out.ctypes.data, caller_ws.ctypes.data if ws else None,
                             ws_bytes if ws else 0, None)
    return rc, out, caller_ws


@pytest.mark.parametrize("poison", POISONS)
def test_well_behaved_call_passes_and_sees_the_poison(poison):
    fake = FakeLib()
    proxy = ContractProxy(fake, Memory("cpu"), poison=poison)
    rc, out, caller_ws = _call(proxy)
    assert rc == 0
    assert (out == np.arange(1, 11)).all()                           # the outputs come back to where the caller asked
    assert (caller_ws == 0x33).all()                                 # the caller's own workspace was never handed over
    assert fake.seen["ws"] % 256 == 0 and fake.seen["out"] % 256 == 0 and fake.seen["ws_bytes"] == 1000
    assert (fake.seen["ws_in"] == poison).all() and (fake.seen["out_in"] == poison).all()
    assert proxy.called["sd_mbd_counts"] == 1 and proxy.guarded_workspaces["sd_mbd_counts"] == 1
    assert ("sd_mbd_counts", poison) in proxy.record


@pytest.mark.parametrize("stray, where", [("past_ws", "past the workspace"), ("far_past_ws", "past the workspace"),
                                          ("before_ws", "before the workspace"), ("past_out", "past output argument 9"),
                                          ("before_out", "before output argument 9")])
def test_a_stray_byte_is_reported(stray, where):
    proxy = ContractProxy(FakeLib(stray), Memory("cpu"), poison=0xA5)
    with pytest.raises(ContractViolation, match=where):
        _call(proxy)


def test_the_offsets_of_a_report_count_from_the_interior():
    with pytest.raises(ContractViolation, match=r"1 byte\(s\) written past the workspace \(1000 bytes\), at offsets 1000 \.\. 1000"):
        _call(ContractProxy(FakeLib("past_ws"), Memory("cpu")))
    with pytest.raises(ContractViolation, match=r"written before the workspace \(1000 bytes\), at offsets -1 \.\. -1"):
        _call(ContractProxy(FakeLib("before_ws"), Memory("cpu")))


def test_a_null_workspace_passes_through():
    fake = FakeLib()
    proxy = ContractProxy(fake, Memory("cpu"))
    rc, out, _ = _call(proxy, ws=False)
    assert rc == 0 and fake.seen["ws"] is None and fake.seen["ws_bytes"] == 0
    assert proxy.guarded_workspaces["sd_mbd_counts"] == 0 and proxy.guarded_outputs["sd_mbd_counts"] == 1
    # a workspace pointer with no bytes is the caller's own, too
    caller_ws = np.zeros(8, dtype=np.uint8)
    proxy.sd_mbd_counts(0, 7, 9, 9, 1, None, 5, 3, 0, out.ctypes.data, caller_ws.ctypes.data, 0, None)
    assert fake.seen["ws"] == caller_ws.ctypes.data


def test_an_entry_point_without_workspace_has_its_output_guarded():
    proxy = ContractProxy(FakeLib(), Memory("cpu"), poison=0xFF)
    out = np.zeros(4)
    assert proxy.sd_l1_depth(0, 10, 2, None, 4, out.ctypes.data, None) == 0
    assert (out == 0.5).all() and proxy.guarded_outputs["sd_l1_depth"] == 1
    assert proxy.sd_last_error() == b""                              # everything else goes straight through


def test_the_word_fill_of_the_stale_gate_cases():
    fake = FakeLib()
    proxy = ContractProxy(fake, Memory("cpu"), poison=0xA5, ws_word=4 << 8 | 0xFF)
    _call(proxy, ws_bytes=1002)
    words = fake.seen["ws_in"][:1000].view(np.uint32)
    assert (words == 0x4FF).all() and list(fake.seen["ws_in"][1000:]) == [0xFF, 0x04]
    assert (fake.seen["out_in"] == 0xA5).all()
    assert ("sd_mbd_counts", ("word", 0x4FF)) in proxy.record


def test_the_guards_are_what_the_issue_asks_for():
    g = Guarded(Memory("cpu"), 100, "x")
    assert g.ptr % 256 == 0 and g.lo >= FRONT_GUARD == 4096 and g.raw.numel() - g.hi >= BACK_GUARD == 1 << 20
    assert (g.raw[:g.lo] == CANARY).all() and (g.raw[g.hi:] == CANARY).all()
    assert CANARY not in POISONS and POISONS == (0x00, 0xFF, 0xA5)


def test_the_table_is_complete():
    """Every entry point that returns int and ends with a stream is in the table or excluded with a reason, and only the
    utility exports are excluded."""
    for name in _native.SIGNATURES:
        if takes_stream(name):
            assert (name in OUTPUTS) != (name in EXCLUDED), f"{name}: in exactly one of the table and the exclusion list"
    for name, reason in EXCLUDED.items():
        assert name in ("sd_malloc", "sd_free", "sd_memset", "sd_stream_synchronize", "sd_set_device") or \
            name.startswith(("sd_memcpy_", "sd_device_")), f"{name} is no utility export"
        assert reason and "\n" not in reason
    for name in OUTPUTS:
        assert takes_stream(name), f"{name} of the table is no entry point with a stream"
    # (sd_memcpy_* end in a pointer, a size and the stream as well: the proxy asks the table first)
    assert all(name in OUTPUTS or name in EXCLUDED for name in _native.SIGNATURES if takes_workspace(name))
    assert compute_symbols() == [n for n in _native.SIGNATURES if takes_stream(n) and n not in EXCLUDED]


def test_every_output_of_the_table_is_a_pointer_in_front_of_the_workspace():
    for name, outs in OUTPUTS.items():
        args = _native.SIGNATURES[name][1]
        end = len(args) - (3 if takes_workspace(name) else 1)
        assert outs, name
        for pos, size in outs:
            assert pos < end and args[pos] is _native._vp, (name, pos)
        assert [pos for pos, _ in outs] == list(range(end - len(outs), end)), f"{name}: the outputs are the last pointers"
