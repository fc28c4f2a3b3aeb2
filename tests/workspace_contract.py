"""The workspace and output contract of include/statdepth_hip.h ("Caller memory"), checked at the ABI boundary.

ContractProxy wraps a ctypes library object and is swapped in for statdepth_amd._native._LIB.  For every compute entry
point it replaces the caller's workspace and outputs by buffers of its own,

    front guard (4 KiB) | exactly the bytes the call may write | back guard (1 MiB)

on a 256-byte aligned pointer, the guards filled with a canary and the interior with the poison of the case; it makes the
call, waits for the stream, asserts that no guard byte changed and copies the outputs to where the caller asked for them.
A null workspace or ws_bytes == 0 passes through unchanged, a null output stays null.

The memory is torch's on either side: `Memory("cpu")` with a fake library of Python callables (the harness's own host
test), `Memory(cuda device, lib)` on the GPU, where the copy to the caller's pointer goes through the library's own
sd_memcpy_h2d.  A plain helper module: no fixtures, no test collection."""
import collections
import ctypes

import numpy as np

from statdepth_amd import _native

FRONT_GUARD = 4096
BACK_GUARD = 1 << 20
CANARY = 0x5C                                 # differs from every poison, top bit clear
POISONS = (0x00, 0xFF, 0xA5)                  # single repeated bytes; in the last two every byte has its top bit set
ALIGN = 256

_vp, _sz, _int = _native._vp, _native._sz, _native._int


class ContractViolation(AssertionError):
    """A call wrote outside the bytes it was given."""


def takes_workspace(name):
    """Does the entry point end (..., ws, ws_bytes, stream)?"""
    res, args = _native.SIGNATURES[name]
    return res is _int and len(args) >= 3 and args[-3:] == [_vp, _sz, _vp]


def takes_stream(name):
    """The rule of the completeness check: returns int and ends with a stream argument."""
    res, args = _native.SIGNATURES[name]
    return res is _int and len(args) >= 1 and args[-1] is _vp


# The outputs of every compute entry point: (position among the C arguments, bytes it spans as a function of the
# arguments).  The extents are the header's: what the call documents as written, nothing rounded up.
def _o(pos, size):
    return (pos, size)


OUTPUTS = {
    # K1 + K2, X T n st sn targets|tbegin m J algo out
    "sd_mbd_counts": [_o(9, lambda a: a[6] * (a[7] - 1) * 8)],
    "sd_mbd_counts_range": [_o(9, lambda a: a[6] * (a[7] - 1) * 8)],
    "sd_mbd_counts_wide": [_o(9, lambda a: a[6] * (a[7] - 1) * 16)],
    "sd_mbd_external_counts": [_o(6, lambda a: a[4] * (a[5] - 1) * 8)],            # X T n Q m J out
    "sd_mbd_subset_counts": [_o(8, lambda a: a[4] * (a[7] - 1) * 8)],              # X T n members nb bs targets J out
    # K3
    "sd_bd_strict_subset_counts": [_o(7, lambda a: a[4] * 8)],                     # X T n members nb bs targets out
    "sd_bd_strict_external_counts": [_o(5, lambda a: a[4] * 8)],                   # X T n Q m out
    "sd_above_below": [_o(7, lambda a: a[6] * a[1] * 2 * 4)],                      # X T n st sn targets m out[m][T][2] u32
    "sd_bd_strict_counts": [_o(7, lambda a: a[6] * 8)],
    "sd_bd_strict_j_counts": [_o(8, lambda a: a[6] * (a[7] - 1) * 8)],
    # point clouds: P n d selection ... out, one value a target
    "sd_l1_depth": [_o(5, lambda a: a[4] * 8)],
    "sd_l1_external_depth": [_o(5, lambda a: a[4] * 8)],
    "sd_l1_subset_depth": [_o(6, lambda a: a[4] * 8)],
    "sd_pointcloud_simplex_counts": [_o(6, lambda a: a[4] * 8)],
    "sd_pointcloud_simplex_external_counts": [_o(6, lambda a: a[4] * 8)],
    "sd_pointcloud_simplex_subset_counts": [_o(7, lambda a: a[4] * 8)],
    "sd_pointcloud_simplex_sampled": [_o(8, lambda a: a[4] * 8)],
    "sd_multi_simplex_counts": [_o(8, lambda a: a[5] * 8)],                        # P n T d targets m relax tol out
    "sd_multi_simplex_sampled": [_o(10, lambda a: a[5] * 8)],
    "sd_multi_band_counts": [_o(6, lambda a: a[5] * 8)],                           # P n T d targets m out
    "sd_multi_band_j_counts": [_o(7, lambda a: a[5] * max(a[6] - 1, 1) * 8)],
    "sd_oja_volume_sums": [_o(5, lambda a: a[4] * 8)],
    "sd_oja_external_volume_sums": [_o(5, lambda a: a[4] * 8)],
    "sd_oja_subset_volume_sums": [_o(6, lambda a: a[4] * 8)],
    "sd_prob_normal_sums": [_o(5, lambda a: a[4] * 8)],                            # mu sigma n targets m out
    "sd_prob_poisson_sums": [_o(6, lambda a: a[5] * 8)],                           # lam T n lim targets m out
    "sd_prob_band_sums": [_o(9, lambda a: a[5] * 8)],                              # mu var T n targets m members bs relax out
    "sd_halfspace_counts": [_o(7, lambda a: a[6] * 8)],                            # P n d U k targets m out
    "sd_halfspace_pairwise_counts": [_o(7, lambda a: a[6] * 8)],
    "sd_halfspace_external_counts": [_o(7, lambda a: a[6] * 8)],
    "sd_halfspace_subset_counts": [_o(8, lambda a: a[6] * 8)],                     # P n d U k members nb bs out
    "sd_halfspace2_counts": [_o(5, lambda a: a[3] * 8)],                           # P n targets m algo out
    "sd_halfspace2_external_counts": [_o(5, lambda a: a[3] * 8)],
    "sd_halfspace2_subset_counts": [_o(6, lambda a: a[3] * 8)],                    # P n members nb bs algo out
    "sd_simplicial2_counts": [_o(5, lambda a: a[3] * 8)],
    "sd_simplicial2_external_counts": [_o(5, lambda a: a[3] * 8)],
    "sd_simplicial2_subset_counts": [_o(6, lambda a: a[3] * 8)],
    "sd_projection_outlyingness": [_o(7, lambda a: a[6] * 8)],
    "sd_projection_external_outlyingness": [_o(7, lambda a: a[6] * 8)],
    "sd_projection_subset_outlyingness": [_o(8, lambda a: a[6] * 8)],
    # curves: X T n st sn targets m ...
    "sd_rank_depth_sums": [_o(8, lambda a: a[6] * 5 * 8)],
    "sd_extremal_counts": [_o(8, lambda a: a[6] * 8)],
    "sd_central_regions": [_o(9, lambda a: a[6] * 2 * a[1] * 8),                   # X T n st sn level L box factor env fence cnt whisker
                           _o(10, lambda a: 2 * a[1] * 8), _o(11, lambda a: a[2] * 2 * 4), _o(12, lambda a: 2 * a[1] * 8)],
    "sd_tvd_sums": [_o(8, lambda a: a[6] * 8), _o(9, lambda a: a[6] * 3 * 8),
                    _o(10, lambda a: max(a[1] - 1, 0) * a[6] * 4)],
    "sd_multi_halfspace_sums": [_o(9, lambda a: a[7] * 2 * 8)],                    # P n T d U k targets m algo out
    "sd_multi_projection_sums": [_o(9, lambda a: a[7] * 2 * 8)],
    "sd_multi_outlyingness_moments": [_o(9, lambda a: a[7] * (a[3] + 1) * 8), _o(10, lambda a: a[2] * 8),
                                      _o(11, lambda a: a[7] * a[2] * a[3] * 8)],
    "sd_curve_sqdist": [_o(7, lambda a: a[6] * a[2] * 8)],
    "sd_curve_sqdist_external": [_o(7, lambda a: a[6] * a[2] * 8)],
    "sd_curve_sqdist_select": [_o(6, lambda a: 8)],                                # X T n st sn k out
    "sd_hmodal_sums": [_o(8, lambda a: a[6] * 8)],
    "sd_hmodal_external_sums": [_o(8, lambda a: a[6] * 8)],
    "sd_spatial_sums": [_o(7, lambda a: a[6] * 8), _o(8, lambda a: a[6] * a[1] * 8)],
    "sd_spatial_external_sums": [_o(7, lambda a: a[6] * 8), _o(8, lambda a: a[6] * a[1] * 8)],
    "sd_lens_counts": [_o(9, lambda a: a[6] * 8)],
    "sd_lens_external_counts": [_o(9, lambda a: a[6] * 8)],
}

# What returns int and ends with a stream (or a pointer that reads as one) and is no compute entry point.
EXCLUDED = {
    "sd_free": "utility: releases an allocation, its only pointer is the allocation",
    "sd_memcpy_h2d": "utility: a copy of the size the caller names",
    "sd_memcpy_d2h": "utility: a copy of the size the caller names",
    "sd_memset": "utility: a fill of the size the caller names",
    "sd_stream_synchronize": "utility: waits for the stream",
}


def compute_symbols():
    """Every entry point the contract covers (the table's keys), in the header's order."""
    return [name for name in _native.SIGNATURES if name in OUTPUTS]


class Memory:
    """Where the guarded buffers live.  device: 'cpu', or a CUDA device with `lib` the real library (for sd_memcpy_h2d)."""

    def __init__(self, device="cpu", lib=None):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.lib = lib

    def empty(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)

    def sync(self):
        if self.device.type == "cuda":
            self.torch.cuda.synchronize(self.device)

    def copy_out(self, dst_ptr, src):
        """src (a uint8 tensor of ours) -> the caller's pointer."""
        host = src.cpu().numpy()
        if self.device.type == "cpu":
            ctypes.memmove(dst_ptr, host.ctypes.data, host.nbytes)
            return
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        _native.check(self.lib.sd_memcpy_h2d(dst_ptr, host.ctypes.data, host.nbytes, stream))
        self.sync()


class Guarded:
    """front guard | nbytes | back guard, the interior on a 256-byte aligned address."""

    def __init__(self, memory, nbytes, what):
        self.what, self.nbytes = what, int(nbytes)
        self.raw = memory.empty(FRONT_GUARD + self.nbytes + BACK_GUARD + ALIGN)
        self.lo = FRONT_GUARD + (-(self.raw.data_ptr() + FRONT_GUARD)) % ALIGN
        self.hi = self.lo + self.nbytes
        self.ptr = self.raw.data_ptr() + self.lo
        assert self.ptr % ALIGN == 0
        self.raw[:self.lo].fill_(CANARY)
        self.raw[self.hi:].fill_(CANARY)

    @property
    def interior(self):
        return self.raw[self.lo:self.hi]

    def poison(self, byte):
        self.interior.fill_(int(byte))

    def poison_words(self, word):
        """The u32 `word` repeated (little endian); a tail of fewer than four bytes takes its first bytes."""
        pattern = np.frombuffer(np.uint32(word).tobytes(), dtype=np.uint8)
        tiled = np.resize(pattern, self.nbytes)
        self.interior.copy_(_as_tensor(self.raw, tiled))

    def check(self, symbol):
        """Offsets in the message count from the first byte of the interior."""
        for side, part, base in (("before", self.raw[:self.lo], -self.lo), ("past", self.raw[self.hi:], self.nbytes)):
            bad = (part != CANARY).nonzero()
            if bad.numel():
                raise ContractViolation(
                    f"{symbol}: {int(bad.numel())} byte(s) written {side} {self.what} ({self.nbytes} bytes), "
                    f"at offsets {int(bad[0]) + base} .. {int(bad[-1]) + base}")


def _as_tensor(like, array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to(like.device)


class ContractProxy:
    """The library object with the contract enforced on every compute entry point.

    poison: the byte the workspace and the outputs hold on entry.  ws_word: instead, a u32 word the WORKSPACE is filled with
    (the stale-gate cases; the outputs keep `poison`).  record: a set that takes (symbol, poison) of every guarded call."""

    def __init__(self, lib, memory, poison=0x00, ws_word=None, record=None):
        self._lib, self._memory, self._poison, self._ws_word = lib, memory, int(poison), ws_word
        self.record = record if record is not None else set()
        self.called = collections.Counter()
        self.guarded_workspaces = collections.Counter()
        self.guarded_outputs = collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in OUTPUTS:
            return fn
        return lambda *args: self._call(name, fn, list(args))

    def _call(self, name, fn, args):
        nargs = len(_native.SIGNATURES[name][1])
        assert len(args) == nargs, f"{name}: {len(args)} arguments for a signature of {nargs}"
        self.called[name] += 1
        regions, outs = [], []
        if takes_workspace(name) and args[-3] and args[-2]:
            ws = Guarded(self._memory, args[-2], "the workspace")
            if self._ws_word is not None:
                ws.poison_words(self._ws_word)
            else:
                ws.poison(self._poison)
            args[-3] = ws.ptr
            regions.append(ws)
            self.guarded_workspaces[name] += 1
        for pos, size in OUTPUTS[name]:
            if not args[pos]:
                continue                                             # an output not asked for
            nbytes = int(size(args))
            if nbytes <= 0:
                continue
            g = Guarded(self._memory, nbytes, f"output argument {pos}")
            g.poison(self._poison)
            outs.append((args[pos], g))
            args[pos] = g.ptr
            regions.append(g)
            self.guarded_outputs[name] += 1
        self._memory.sync()
        rc = fn(*args)
        self._memory.sync()
        for g in regions:
            g.check(name)
        if rc == 0:
            for dst, g in outs:
                self._memory.copy_out(dst, g.interior)
        self.record.add((name, self._poison if self._ws_word is None else ("word", self._ws_word)))
        return rc
