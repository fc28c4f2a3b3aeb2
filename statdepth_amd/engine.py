"""Host-side driver of the HIP kernels: ndarray / torch tensor in, integer counts out.

Everything numerical happens in libstatdepth_hip.so; this module moves data to HBM
(torch is the allocator / stream provider), sizes workspaces and calls the C ABI.
"""
import threading

import numpy as np

from . import _native
from ._native import ALGOS, check

_torch = None


def torch():
    global _torch
    if _torch is None:
        import torch as t
        _torch = t
    return _torch


def _lib():
    """The C library, torch imported first: imported after the library has started the HIP runtime, torch finds no
    device."""
    torch()
    return _native.require_device()


def _device(device=None):
    t = torch()
    _lib()
    if not t.cuda.is_available():
        raise RuntimeError("statdepth_amd: torch reports no ROCm device")
    if device is None:
        return t.device("cuda", t.cuda.current_device())
    return t.device(device)


def _stream_ptr(dev):
    return torch().cuda.current_stream(dev).cuda_stream


class DeviceMatrix:
    """A T x n fp64 data set resident in HBM in one of the two pandas layouts.

    `tensor` is a 2-D torch tensor whose logical shape is (T, n); strides (in
    elements) describe either layout, exactly what sd_* expect as (st, sn).
    """

    def __init__(self, tensor):
        t = torch()
        assert tensor.dim() == 2 and tensor.dtype == t.float64 and tensor.is_cuda
        st, sn = tensor.stride()
        T, n = tensor.shape
        if not ((sn == 1 and st == n) or (st == 1 and sn == T) or T == 1 or n == 1):
            tensor = tensor.contiguous()
            st, sn = tensor.stride()
        if n == 1 or T == 1:      # degenerate strides: normalise to time-major
            tensor = tensor.contiguous()
            st, sn = n, 1
        self.tensor = tensor
        self.T, self.n, self.st, self.sn = int(T), int(n), int(st), int(sn)

    @property
    def device(self):
        return self.tensor.device


def to_device_matrix(X, device=None):
    """ndarray (T, n) in either memory order, or a CUDA tensor -> DeviceMatrix (no layout change)."""
    t = torch()
    if isinstance(X, DeviceMatrix):
        return X
    if isinstance(X, t.Tensor):
        if not X.is_cuda:
            X = X.to(_device(device))
        return DeviceMatrix(X.to(t.float64))
    dev = _device(device)
    A = np.asarray(X, dtype=np.float64)
    if A.ndim != 2:
        raise ValueError("expected a 2-D array (timepoints x curves)")
    if A.flags.c_contiguous or not A.flags.f_contiguous:
        A = np.ascontiguousarray(A)
        return DeviceMatrix(t.from_numpy(A).to(dev))
    # F-contiguous (column-built DataFrame): ship the bytes as they lie, view as (T, n)
    return DeviceMatrix(t.from_numpy(A.T).to(dev).t())


# One grow-only scratch buffer per (device, stream, host thread), reused by every call (the C ABI takes the workspace as an
# argument, reads nothing from it that the same call has not written and keeps nothing in it between calls -- "Caller memory"
# in include/statdepth_hip.h, which also lets every output be torch.empty): a repeated call of the same shape pays no
# allocation and no allocator round trip.
# The launchers are multi-launch pipelines with live state in the buffer between their launches, and ctypes releases the
# GIL: two host threads on ONE stream must not share a buffer (their launches may interleave), hence the thread in the key.
# Results handed out with return_tensor=True are separate tensors and stay valid.  Buffers above _WS_KEEP bytes are handed
# out once and not kept (strict depth at large n asks for GiBs); at most _WS_SLOTS buffers are kept, least recently used
# first out (side streams and worker threads that are gone).
_WS_KEEP = 2 << 30
_WS_SLOTS = 8
_ws_cache = {}
_ws_lock = threading.Lock()


def _ws_key(dev):
    # per (device, stream, thread): calls of one thread on one stream run in order and may share the buffer
    t = torch()
    idx = dev.index if dev.index is not None else t.cuda.current_device()
    return (idx, t.cuda.current_stream(dev).cuda_stream, threading.get_ident())


def _workspace(dev, nbytes):
    t = torch()
    nbytes = max(int(nbytes), 8)
    key = _ws_key(dev)
    with _ws_lock:
        buf = _ws_cache.pop(key, None)
        if buf is not None and buf.numel() >= nbytes:
            _ws_cache[key] = buf                                      # most recently used last
            return buf
    del buf                                                           # the smaller buffer goes back before the larger one is asked for
    new = t.empty(nbytes, dtype=t.uint8, device=dev)
    if nbytes <= _WS_KEEP:
        with _ws_lock:
            _ws_cache[key] = new
            while len(_ws_cache) > _WS_SLOTS:
                _ws_cache.pop(next(iter(_ws_cache)))
    return new


def release_workspace():
    """Drop the cached scratch buffers (they are plain torch tensors; the caching allocator gets them back)."""
    with _ws_lock:
        _ws_cache.clear()


def _upload(A, ndim, dev):
    """ndarray or tensor -> contiguous fp64 tensor with `ndim` dimensions on dev (as it is, when it already is one)."""
    t = torch()
    if not isinstance(A, t.Tensor):
        A = t.from_numpy(np.ascontiguousarray(np.asarray(A, dtype=np.float64)))
    if A.dim() != ndim:
        raise ValueError(f"expected a {ndim}-D array")
    return A.to(dev, t.float64).contiguous()


# Index arrays go to the device as they are and the kernels read X through them: both helpers refuse, on the host and
# before the upload, what would read outside the data set.
def _targets_dev(targets, n, dev, dtype=np.int64):
    """(tensor, m, pointer) of the target indices on dev; targets=None means all n (NULL pointer)."""
    t = torch()
    if targets is None:
        return None, n, 0
    tg = np.ascontiguousarray(np.asarray(targets, dtype=dtype))
    if tg.ndim != 1:
        raise ValueError("targets must be 1-D")
    if len(tg) and (tg.min() < 0 or tg.max() >= n):
        raise IndexError("target index out of range")
    td = t.from_numpy(tg).to(dev)
    return td, len(tg), td.data_ptr()


def _members_dev(members, dev, n, rows=None, trailing_padding=False):
    """(tensor, nb, bs) of the block members on dev: nb blocks of bs indices, -1 padded.  rows: the number of blocks
    the caller has targets for.  trailing_padding: the point-cloud block form, whose kernels take a block's members up to
    its first -1 and its target from the last of them -- a -1 in front of a member is refused."""
    t = torch()
    mem = np.ascontiguousarray(np.asarray(members, dtype=np.int32))
    if mem.ndim != 2:
        raise ValueError("members must be 2-D (blocks x block size, -1 padded, target last)")
    if rows is not None and mem.shape[0] != rows:
        raise ValueError("members must have one row (block) per target")
    lowest = int(mem.min()) if mem.size else 0
    if mem.size and (lowest < -1 or int(mem.max()) >= n):
        raise IndexError("block member index out of range (valid: -1 padding, 0 .. n-1)")
    if trailing_padding and lowest < 0:                              # (an array without padding is not read again)
        pad = mem.ravel() < 0
        gap = pad[:-1] > pad[1:]                                      # a -1 with a member behind it ...
        gap[mem.shape[1] - 1::mem.shape[1]] = False                   # ... in the same block
        if bool(gap.any()):
            raise IndexError("block members must come first and the -1 padding last")
    return t.from_numpy(mem).to(dev), mem.shape[0], mem.shape[1]


def _sized(dev, nbytes):
    """(buffer, bytes) for an entry point that asks for nbytes of workspace."""
    return _workspace(dev, nbytes), int(nbytes)


_OUT = object()                                                      # the place of `out` among _launch's args, unless it is the last


def _launch(dev, fn, out, *args, workspace=None, return_tensor=False):
    """fn(*args, out, [ws, ws_bytes,] stream) on dev's current stream, out at the place of _OUT where args name one; returns
    out as an ndarray, or the tensor itself with return_tensor.  Nothing is launched when out has no rows.  workspace:
    None, or a function of no arguments returning (buffer, bytes), asked for only when there is something to launch; a buffer
    of None is passed as a null pointer."""
    t = torch()
    if out.shape[0]:
        ws = workspace() if workspace is not None else None
        tail = (ws[0].data_ptr() if ws[0] is not None else None, ws[1]) if ws is not None else ()
        head = args if any(a is _OUT for a in args) else (*args, _OUT)
        with t.cuda.device(dev):
            check(fn(*(out.data_ptr() if a is _OUT else a for a in head), *tail, _stream_ptr(dev)))
    return out if return_tensor else out.cpu().numpy()


def _mbd_counts(lib, fn, M, first, m, J, algo, return_tensor):
    """sd_mbd_counts / sd_mbd_counts_range: `first` is the targets' pointer, or the first target of the block."""
    t = torch()
    dev = M.device
    a = ALGOS[algo] if isinstance(algo, str) else int(algo)
    out = t.empty((m, J - 1), dtype=t.int64, device=dev)
    return _launch(dev, fn, out, M.tensor.data_ptr(), M.T, M.n, M.st, M.sn, first, m, J, a,
                   workspace=lambda: _sized(dev, lib.sd_mbd_workspace_bytes(M.T, M.n, M.st, M.sn, m, J, a)),
                   return_tensor=return_tensor)


def mbd_counts(X, targets=None, J=2, algo="auto", device=None, return_tensor=False):
    """int64[m, J-1]: sum over t of contained j-bands per target (sd_mbd_counts)."""
    lib = _lib()
    M = to_device_matrix(X, device)
    td, m, tp = _targets_dev(targets, M.n, M.device)
    return _mbd_counts(lib, lib.sd_mbd_counts, M, tp, m, J, algo, return_tensor)


def mbd_counts_wide(X, targets=None, J=2, algo="auto", device=None):
    """object[m, J-1] of Python ints: the totals of mbd_counts beyond int64 (sd_mbd_counts_wide, two 64-bit limbs)."""
    t = torch()
    lib = _lib()
    M = to_device_matrix(X, device)
    dev = M.device
    td, m, tp = _targets_dev(targets, M.n, dev)
    a = ALGOS[algo] if isinstance(algo, str) else int(algo)
    out = t.empty((m, J - 1, 2), dtype=t.int64, device=dev)
    limbs = _launch(dev, lib.sd_mbd_counts_wide, out, M.tensor.data_ptr(), M.T, M.n, M.st, M.sn, tp, m, J, a,
                    workspace=lambda: _sized(dev, lib.sd_mbd_wide_workspace_bytes(M.T, M.n, M.st, M.sn, m, J, a)))
    limbs = limbs.astype(np.uint64)
    res = np.empty((m, J - 1), dtype=object)
    for q in range(m):
        for j in range(J - 1):
            res[q, j] = (int(limbs[q, j, 1]) << 64) | int(limbs[q, j, 0])
    return res


def mbd_counts_range(X, target_begin, m, J=2, algo="auto", device=None, return_tensor=False):
    """Totals for the contiguous target block [target_begin, target_begin + m) (sd_mbd_counts_range)."""
    lib = _lib()
    M = to_device_matrix(X, device)
    return _mbd_counts(lib, lib.sd_mbd_counts_range, M, int(target_begin), int(m), J, algo, return_tensor)


def _external_curves(fn, X, Q, device, *extra, outputs, ws_bytes=None, family=None, variant=None):
    """fn(X, T, n, [st, sn,] Q, m, *extra, *outputs, ws, ws_bytes, stream) for the m columns of Q (T x m) against the n columns
    of X, which goes up time-major.  outputs(t, dev, T, n, m): the output tensors in the order of the C signature, None for one
    not asked for (fn gets NULL there); returned as ndarrays.  family None: ws_bytes(T, n, m) is the workspace size.  A
    family of _CURVE_FAMILIES: fn takes (st, sn) behind n, and ws_bytes is the size to run with (None: what the family
    recommends for `variant`)."""
    t = torch()
    dev = _device(device)
    Xd, Qd = _upload(X, 2, dev), _upload(Q, 2, dev)
    T, n = Xd.shape
    if Qd.shape[0] != T:
        raise ValueError("Q must have the same number of timepoints as X")
    m = Qd.shape[1]
    outs = outputs(t, dev, T, n, m)
    if family is None:
        strides, size = (), lambda: ws_bytes(T, n, m)
    else:
        strides = (n, 1)
        size = lambda: _curve_size(family, "workspace_bytes", T, n, strides, m, variant) if ws_bytes is None else ws_bytes
    _launch(dev, fn, outs[0], Xd.data_ptr(), T, n, *strides, Qd.data_ptr(), m, *extra, _OUT,
            *(o.data_ptr() if o is not None and o.numel() else None for o in outs[1:]),
            workspace=lambda: _sized(dev, size()), return_tensor=True)
    return [o.cpu().numpy() if o is not None else None for o in outs]


def mbd_external_counts(X, Q, J=2, device=None):
    """int64[m, J-1]: band totals of the m columns of Q (T x m) w.r.t. the n columns of X (sd_mbd_external_counts)."""
    lib = _lib()
    return _external_curves(lib.sd_mbd_external_counts, X, Q, device, J,
                            outputs=lambda t, dev, T, n, m: [t.empty((m, J - 1), dtype=t.int64, device=dev)],
                            ws_bytes=lambda T, n, m: lib.sd_mbd_external_workspace_bytes(T, n, m, J) + 1024)[0]


def bd_strict_external_counts(X, Q, device=None):
    """int64[m]: pairs of X's n columns whose band contains column q of Q (T x m) at every t (sd_bd_strict_external_counts)."""
    lib = _lib()
    return _external_curves(lib.sd_bd_strict_external_counts, X, Q, device,
                            outputs=lambda t, dev, T, n, m: [t.empty((m,), dtype=t.int64, device=dev)],
                            ws_bytes=lib.sd_bd_strict_external_workspace_bytes)[0]


def _subset_curves(fn, cols, X, members, targets, device, *extra, ws_bytes=None):
    """fn(X, T, n, members, nb, bs, targets, *extra, out, [ws, ws_bytes,] stream) for targets[k] inside the curves
    members[k].  out: int64 (nb, *cols); ws_bytes(T, nb, bs): the workspace size, where fn takes one."""
    t = torch()
    dev = _device(device)
    Xd = _upload(X, 2, dev)
    T, n = Xd.shape
    td, m, tp = _targets_dev(targets, n, dev, np.int32)
    md, nb, bs = _members_dev(members, dev, n, rows=m)
    out = t.empty((nb, *cols), dtype=t.int64, device=dev)
    workspace = (lambda: _sized(dev, ws_bytes(T, nb, bs))) if ws_bytes is not None else None
    return _launch(dev, fn, out, Xd.data_ptr(), T, n, md.data_ptr(), nb, bs, tp, *extra, workspace=workspace)


def mbd_subset_counts(X, members, targets, J=2, device=None):
    """int64[nb, J-1]: band totals of targets[k] inside the curves members[k] (-1 padded) -- sd_mbd_subset_counts."""
    lib = _lib()
    return _subset_curves(lib.sd_mbd_subset_counts, (J - 1,), X, members, targets, device, J)


def bd_strict_subset_supported(T, bs):
    """Does a block of `bs` curves x T timepoints fit sd_bd_strict_subset_counts (masks in LDS)?"""
    return bool(_lib().sd_bd_strict_subset_supported(int(T), int(bs)))


def bd_strict_subset_counts(X, members, targets, device=None):
    """int64[nb]: pairs of members[k]'s other curves (-1 padded) containing targets[k] at every t (sd_bd_strict_subset_counts)."""
    lib = _lib()
    return _subset_curves(lib.sd_bd_strict_subset_counts, (), X, members, targets, device,
                          ws_bytes=lib.sd_bd_strict_subset_workspace_bytes)


def above_below(X, targets=None, device=None):
    """uint32 -> int64 [m, T, 2] strictly-above / strictly-below counts (sd_above_below)."""
    t = torch()
    lib = _lib()
    M = to_device_matrix(X, device)
    dev = M.device
    td, m, tp = _targets_dev(targets, M.n, dev)
    out = t.empty((m, M.T, 2), dtype=t.int32, device=dev)
    ab = _launch(dev, lib.sd_above_below, out, M.tensor.data_ptr(), M.T, M.n, M.st, M.sn, tp, m,
                 workspace=lambda: _sized(dev, M.T * M.n * 8 + 1024))
    return ab.astype(np.int64) & 0xFFFFFFFF


def _strict_workspace(lib, dev, M, m, J, budget=None):
    """(buffer, bytes) for sd_bd_strict_j_counts.  The recommended size holds the masks of a large batch of targets (GiBs
    at large n); the launcher sizes its batches to whatever it is given, so when the device is short of memory -- the
    caller keeps other tensors there -- the request shrinks towards the floor of one target per batch instead of failing."""
    t = torch()
    if J == 2 and 6 <= M.T <= 8 and not bool(t.isnan(M.tensor).any()):
        # NaN-free series of 6 ... 8 timepoints are counted through state classes: a flag, none of the mask pipeline's GiBs
        # (include/statdepth_hip.h, K3; the launcher checks for NaN itself and would refuse this size if there were any)
        small = int(lib.sd_bd_strict_nanfree_workspace_bytes(M.T, M.n, M.st, M.sn, m))
        return _workspace(dev, small), small
    want = int(lib.sd_bd_strict_j_workspace_bytes(M.T, M.n, M.st, M.sn, m, J))
    floor = int(lib.sd_bd_strict_min_workspace_bytes(M.T, M.n, M.st, M.sn, m, J))
    if budget is not None:
        want = max(floor, min(want, int(budget)))
    else:
        with t.cuda.device(dev):
            free, _ = t.cuda.mem_get_info()
        cached = _ws_cache.get(_ws_key(dev))
        have = free + t.cuda.memory_reserved(dev) - t.cuda.memory_allocated(dev) + (cached.numel() if cached is not None else 0)
        want = max(floor, min(want, int(have * 0.8)))
    while True:
        try:
            return _workspace(dev, want), want
        except t.cuda.OutOfMemoryError:
            if want <= floor:
                raise
            release_workspace()
            t.cuda.empty_cache()
            want = max(floor, want // 2)


def bd_strict_counts(X, targets=None, J=2, device=None, workspace_budget=None):
    """int64[m, J-1]: j-subsets whose band contains the target at every t (sd_bd_strict_j_counts).
    workspace_budget: upper bound in bytes for the scratch buffer (default: the recommended size, or what the device has
    free); never below the floor of one target per batch."""
    t = torch()
    lib = _lib()
    M = to_device_matrix(X, device)
    dev = M.device
    td, m, tp = _targets_dev(targets, M.n, dev)
    out = t.empty((m, J - 1), dtype=t.int64, device=dev)
    return _launch(dev, lib.sd_bd_strict_j_counts, out, M.tensor.data_ptr(), M.T, M.n, M.st, M.sn, tp, m, J,
                   workspace=lambda: _strict_workspace(lib, dev, M, m, J, workspace_budget))


RANK_DEPTH_ALGOS = {"auto": 0, "image": 1, "sort": 2}
TVD_ALGOS = {"auto": 0, "lds": 1, "pairwise": 2}
CURVE_DIST_WHAT = {"sqdist": 0, "hmodal": 1, "select": 2}
# The curve families with a workspace plan, by the prefix of sd_<family>_workspace_bytes, _min_workspace_bytes and
# _<rows or targets>_per_batch: the names of the algo that follows m in these and in the family's entry points (None: it has
# none), and whether a `what` of CURVE_DIST_WHAT follows m in the size functions alone.  The `variant` of the helpers below is
# that algo or `what`.
_CURVE_FAMILIES = {"rank_depth": (RANK_DEPTH_ALGOS, False), "extremal": (RANK_DEPTH_ALGOS, False), "tvd": (TVD_ALGOS, False),
                   "curve_sqdist": (None, True), "spatial": (None, False), "lens": (None, False)}


def _variant(family, variant):
    """What follows m in the family's size functions: (the number of the algo or of the `what`,), or ()."""
    algos, what = _CURVE_FAMILIES[family]
    if what:
        return (CURVE_DIST_WHAT[variant],)
    if algos is None:
        return ()
    if isinstance(variant, str) and variant not in algos:
        raise ValueError(f"algo must be one of {sorted(algos)}, got {variant!r}")
    return (algos[variant] if isinstance(variant, str) else int(variant),)


def _strides(T, n, curve_major):
    """(st, sn) of a T x n matrix: curve-major (F-contiguous), or time-major, which a single row or column always is."""
    return (1, T) if curve_major and T > 1 and n > 1 else (n, 1)


def _curve_size(family, name, T, n, strides, m, variant, *more):
    """sd_<family>_<name>(T, n, st, sn, m, [algo or what,] *more); m None: all n."""
    fn, T, n = getattr(_native.load(), f"sd_{family}_{name}"), int(T), int(n)
    return int(fn(T, n, *strides, n if m is None else int(m), *_variant(family, variant), *more))


def _curve_sizes(family, T, n, variant, curve_major, m=None):
    """(recommended, floor) workspace sizes of the family for a T x n matrix and m targets."""
    st = _strides(int(T), int(n), curve_major)
    return tuple(_curve_size(family, name, T, n, st, m, variant) for name in ("workspace_bytes", "min_workspace_bytes"))


def _curve_per_batch(family, unit, T, n, ws_bytes, variant, curve_major, m=None):
    """The rows or targets (`unit`) a batch of the family takes with ws_bytes of workspace."""
    return _curve_size(family, f"{unit}_per_batch", T, n, _strides(int(T), int(n), curve_major), m, variant, int(ws_bytes))


def _curves(fn, family, variant, X, targets, device, own, ws_bytes, outputs):
    """lib.<fn>(X, T, n, st, sn, targets, m, [algo,] *own, *outputs, ws, ws_bytes, stream) with ws_bytes of workspace (None:
    what the family of _CURVE_FAMILIES recommends for `variant`).  algo: the variant's number, where the family has algos.
    own: the call's own arguments between there and the outputs.  outputs(t, dev, M, m): the output tensors in the order of
    the C signature, None for one not asked for; nothing is launched when the first has no rows.  Returns them as ndarrays."""
    t = torch()
    lib = _lib()
    M = to_device_matrix(X, device)
    dev = M.device
    algo = _variant(family, variant) if _CURVE_FAMILIES[family][0] is not None else ()
    td, m, tp = _targets_dev(targets, M.n, dev)
    outs = outputs(t, dev, M, m)
    _launch(dev, getattr(lib, fn), outs[0], M.tensor.data_ptr(), M.T, M.n, M.st, M.sn, tp, m, *algo, *own, _OUT,
            *(o.data_ptr() if o is not None and o.numel() else None for o in outs[1:]),
            workspace=lambda: _sized(dev, _curve_size(family, "workspace_bytes", M.T, M.n, (M.st, M.sn), m, variant)
                                     if ws_bytes is None else ws_bytes),
            return_tensor=True)
    return [o.cpu().numpy() if o is not None else None for o in outs]


def rank_depth_workspace_bytes(T, n, algo="auto", curve_major=False):
    """(recommended, floor) workspace sizes of sd_rank_depth_sums for a T x n matrix; the floor holds one row per batch.
    curve_major: the matrix is F-contiguous and takes a time-major copy in the workspace as well."""
    return _curve_sizes("rank_depth", T, n, algo, curve_major)


def rank_depth_rows_per_batch(T, n, ws_bytes, algo="auto", curve_major=False):
    """Rows of the matrix a batch (image route) or a chunk (sort route) of sd_rank_depth_sums takes with ws_bytes of
    workspace; 0 below the floor.  At the recommended size this is all T rows whenever T is within the route's caps."""
    return _curve_per_batch("rank_depth", "rows", T, n, ws_bytes, algo, curve_major)


def rank_depth_sums(X, targets=None, device=None, algo="auto", ws_bytes=None):
    """int64[m, 5]: the records (SA, SB, SF, SM, MM) of the integrated rank depths (sd_rank_depth_sums) -- per target the
    sums over t of A (others strictly above), of B (strictly below), of |2A - n| and of max(A, B), and the maximum over t
    of max(A, B).  X must not hold NaN (the depth layer checks; this function takes its array as it is).  algo: 'auto',
    'image' (n <= 16 384) or 'sort', or their numbers 0, 1, 2.  ws_bytes: the workspace size to run with (default: the
    recommended one); the records do not depend on it, below the floor the library refuses."""
    return _curves("sd_rank_depth_sums", "rank_depth", algo, X, targets, device, (), ws_bytes,
                   lambda t, dev, M, m: [t.empty((m, 5), dtype=t.int64, device=dev)])[0]


def extremal_workspace_bytes(T, n, algo="auto", curve_major=False):
    """(recommended, floor) workspace sizes of sd_extremal_counts for a T x n matrix: the extremity matrix (4 T n bytes)
    and the heads (8 n) in front of the batch of sd_rank_depth_sums; the floor holds one row per batch.  (0, 0) for a
    shape or algo the call refuses.  curve_major: the matrix is F-contiguous and takes a time-major copy as well."""
    return _curve_sizes("extremal", T, n, algo, curve_major)


def extremal_counts(X, targets=None, device=None, algo="auto", ws_bytes=None):
    """int64[m]: G of the extremal depth (sd_extremal_counts) -- per target the number of sample curves, itself included,
    whose descending-sorted vector of pointwise extremities |A - B| is lexicographically at least the target's; the depth
    is G / n.  X must not hold NaN (the depth layer checks; this function takes its array as it is).  targets: indices of
    sample curves (None: all).  algo and ws_bytes as for rank_depth_sums; the counts do not depend on ws_bytes."""
    return _curves("sd_extremal_counts", "extremal", algo, X, targets, device, (), ws_bytes,
                   lambda t, dev, M, m: [t.empty((m,), dtype=t.int64, device=dev)])[0]


def tvd_workspace_bytes(T, n, algo="auto", curve_major=False, m=None):
    """(recommended, floor) workspace sizes of sd_tvd_sums for a T x n matrix and m targets (default: all n); the floor holds
    one row per batch.  (0, 0) for a shape or algo the call refuses.  curve_major: the matrix is F-contiguous and takes a
    time-major copy in the workspace as well."""
    return _curve_sizes("tvd", T, n, algo, curve_major, m)


def tvd_rows_per_batch(T, n, ws_bytes, algo="auto", curve_major=False, m=None):
    """Rows of the matrix a batch of sd_tvd_sums takes with ws_bytes of workspace (all T on the pairwise route); 0 below
    the floor."""
    return _curve_per_batch("tvd", "rows", T, n, ws_bytes, algo, curve_major, m)


def tvd_sums(X, targets=None, device=None, algo="auto", ws_bytes=None, counts=False):
    """(sd_sum int64[m], shape float64[m, 3]) of the total variation depth and the shape similarity (sd_tvd_sums), and with
    counts=True a third entry, uint32[T - 1, m].  Per target q, with a_t = #{j : X[t][j] <= X[t][q]} and c_t = #{j : X[t-1][j]
    <= X[t-1][q] and X[t][j] <= X[t][q]} over the whole sample: sd_sum = sum_t a_t (n - a_t); shape = (SS, SN, SW), the sums over
    t >= 1 of S_t, |D_t| S_t and |D_t|, S_t the squared phi coefficient of (a_s, a_t, c_t) (depth/calculations/_shape.py) and
    D_t = X[t][q] - X[t-1][q]; counts[t - 1][q] = c_t.  X must not hold NaN (the depth layer checks; this function takes its
    array as it is).  algo: 'auto', 'lds' (n <= 16 384) or 'pairwise', or their numbers 0, 1, 2.  ws_bytes: the workspace
    size to run with (default: the recommended one); the results do not depend on it, below the floor the library
    refuses."""
    sd, shape, cnt = _curves("sd_tvd_sums", "tvd", algo, X, targets, device, (), ws_bytes, lambda t, dev, M, m: [
        t.empty((m,), dtype=t.int64, device=dev), t.empty((m, 3), dtype=t.float64, device=dev),
        t.empty((max(M.T - 1, 0), m), dtype=t.int32, device=dev) if counts else None])
    return (sd, shape, cnt.view(np.uint32)) if counts else (sd, shape)


def curve_sqdist_workspace_bytes(T, n, what="sqdist", curve_major=False, m=None):
    """(recommended, floor) workspace sizes of the K20 calls for a T x n matrix and m targets (default: all n).  what:
    'sqdist' (nothing but the time-major copy of a curve-major matrix: both may be 0), 'hmodal' (the tiles' partial sums of
    a batch of targets; the floor holds one block of 128) or 'select' (histogram and state; the recommended size also holds
    the n x n matrix where that is at most 1 GiB).  (0, 0) for a shape the calls refuse."""
    return _curve_sizes("curve_sqdist", T, n, what, curve_major, m)


def curve_sqdist_targets_per_batch(T, n, ws_bytes, what="sqdist", curve_major=False, m=None):
    """Targets a batch of a K20 call takes with ws_bytes of workspace (all of them for 'sqdist' and 'select'); 0 below the
    floor."""
    return _curve_per_batch("curve_sqdist", "targets", T, n, ws_bytes, what, curve_major, m)


def _bandwidth_factor(g):
    g = float(g)
    if not (0.0 < g < float("inf")):
        raise ValueError(f"g = 1 / (2 h^2) must be positive and finite, got {g!r}")
    return g


def curve_sqdist(X, targets=None, device=None, ws_bytes=None):
    """float64[m, n]: the squared L2 distances of the targets (indices of sample curves; None: all) to the n columns of X
    (sd_curve_sqdist): per pair one accumulator over ascending t, d = x[t] - y[t], acc = fma(d, d, acc).  The matrix is
    bitwise symmetric with a +0.0 diagonal.  X must be finite with |x| <= 2^480 (the depth layer checks; this function takes
    its array as it is).  ws_bytes: the workspace size to run with (default: the recommended one); below the floor the
    library refuses."""
    return _curves("sd_curve_sqdist", "curve_sqdist", "sqdist", X, targets, device, (), ws_bytes,
                   lambda t, dev, M, m: [t.empty((m, M.n), dtype=t.float64, device=dev)])[0]


def curve_sqdist_external(X, Q, device=None, ws_bytes=None):
    """float64[m, n]: the squared L2 distances of the m columns of Q (T x m) to the n columns of X
    (sd_curve_sqdist_external); the arithmetic of curve_sqdist.  X goes up time-major, so no workspace is needed."""
    return _external_curves(_lib().sd_curve_sqdist_external, X, Q, device, ws_bytes=ws_bytes, family="curve_sqdist",
                            variant="sqdist", outputs=lambda t, dev, T, n, m: [t.empty((m, n), dtype=t.float64, device=dev)])[0]


def curve_sqdist_select(X, k, device=None, ws_bytes=None):
    """The k-th smallest (k = 1 .. n (n - 1) / 2) squared L2 distance over the pairs i < j of the columns of X, as a float
    (sd_curve_sqdist_select): a radix descent on the distances' 64-bit images.  With the recommended workspace the matrix
    is kept (where it is at most 1 GiB), with less every pass recomputes it; the result is the same."""
    n = int(np.shape(X)[1]) if not isinstance(X, DeviceMatrix) else X.n
    k = int(k)
    if not 1 <= k <= n * (n - 1) // 2:
        raise ValueError(f"k must lie in [1, {n * (n - 1) // 2}], the pairs of {n} curves, got {k}")
    t = torch()
    lib = _lib()
    M = to_device_matrix(X, device)
    dev = M.device
    out = t.empty((1,), dtype=t.float64, device=dev)
    size = lambda: _curve_size("curve_sqdist", "workspace_bytes", M.T, M.n, (M.st, M.sn), None, "select")
    return float(_launch(dev, lib.sd_curve_sqdist_select, out, M.tensor.data_ptr(), M.T, M.n, M.st, M.sn, k,
                         workspace=lambda: _sized(dev, size() if ws_bytes is None else ws_bytes))[0])


def hmodal_sums(X, g, targets=None, device=None, ws_bytes=None):
    """float64[m]: S = sum_j exp(-(D2[q][j] * g)) over all n columns of X per target (sd_hmodal_sums), D2 as in
    curve_sqdist and g = 1 / (2 h^2); the target's own term is 1.0.  The order of the sum depends on n alone, so S of a
    target holds the same bits whatever the targets, the layout of X or ws_bytes.  targets, ws_bytes and the contract on X
    as for curve_sqdist."""
    return _curves("sd_hmodal_sums", "curve_sqdist", "hmodal", X, targets, device, (_bandwidth_factor(g),), ws_bytes,
                   lambda t, dev, M, m: [t.empty((m,), dtype=t.float64, device=dev)])[0]


def hmodal_external_sums(X, Q, g, device=None, ws_bytes=None):
    """float64[m]: the sums of hmodal_sums for the m columns of Q (T x m) against the n columns of X
    (sd_hmodal_external_sums); no term is the target's own."""
    return _external_curves(_lib().sd_hmodal_external_sums, X, Q, device, _bandwidth_factor(g), ws_bytes=ws_bytes,
                            family="curve_sqdist", variant="hmodal",
                            outputs=lambda t, dev, T, n, m: [t.empty((m,), dtype=t.float64, device=dev)])[0]


def spatial_workspace_bytes(T, n, curve_major=False, m=None):
    """(recommended, floor) workspace sizes of sd_spatial_sums for a T x n matrix and m targets (default: all n): the weights
    (8 n bytes a target) and the field (8 T bytes a target) of a batch of whole blocks of 128 targets, behind the time-major
    copy of a curve-major matrix.  The floor holds one block; the recommended size holds all targets, up to 8 GiB of weights
    a batch.  (0, 0) where T < 1, n < 2 or m < 0."""
    return _curve_sizes("spatial", T, n, None, curve_major, m)


def spatial_targets_per_batch(T, n, ws_bytes, curve_major=False, m=None):
    """Targets a batch of sd_spatial_sums takes with ws_bytes of workspace; 0 below the floor."""
    return _curve_per_batch("spatial", "targets", T, n, ws_bytes, None, curve_major, m)


def spatial_time_tile(T, targets, device=None):
    """Timepoints of the tile that the sum kernel of sd_spatial_sums takes for a batch of `targets` targets on the device's
    current stream: 64, or 32 where the wider tile would give fewer than two workgroups per compute unit.  The results do
    not depend on it."""
    lib = _lib()
    dev = _device(device)
    with torch().cuda.device(dev):
        return int(lib.sd_spatial_time_tile(int(T), int(targets), _stream_ptr(dev)))


def spatial_sums(X, targets=None, device=None, ws_bytes=None, field=False):
    """float64[m]: S = |E|^2 of the functional spatial depth per target (sd_spatial_sums), and with field=True the pair
    (S, E), E float64[m, T].  E[t] = sum_j w_j (x[t] - x_j[t]) over all n columns of X in ascending j with one fma per term,
    w_j = 1 / sqrt(D2_j) on curve_sqdist's D2, and w_j = 0.0 where D2_j == 0.0: a coincident curve (the target itself, a
    duplicate) adds nothing; S = sum_t E[t]^2 in ascending t with one fma per term.  The depth is 1 - sqrt(S) / n.  S and E of
    a target hold the same bits whatever the targets, the layout of X or ws_bytes.  targets, ws_bytes and the contract on X
    as for curve_sqdist."""
    S, E = _curves("sd_spatial_sums", "spatial", None, X, targets, device, (), ws_bytes, lambda t, dev, M, m: [
        t.empty((m,), dtype=t.float64, device=dev), t.empty((m, M.T), dtype=t.float64, device=dev) if field else None])
    return (S, E) if field else S


def spatial_external_sums(X, Q, device=None, ws_bytes=None, field=False):
    """float64[m], or (S, E) with field=True: the sums of spatial_sums for the m columns of Q (T x m) against the n columns
    of X (sd_spatial_external_sums).  The depth is 1 - sqrt(S) / (n + 1): the sample it refers to includes the target.  A
    column of Q equal to a sample curve gives that curve's S."""
    outputs = lambda t, dev, T, n, m: [t.empty((m,), dtype=t.float64, device=dev),
                                       t.empty((m, T), dtype=t.float64, device=dev) if field else None]
    S, E = _external_curves(_lib().sd_spatial_external_sums, X, Q, device, ws_bytes=ws_bytes, family="spatial", outputs=outputs)
    return (S, E) if field else S


LENS_MAX_N = 16384                                                   # curves whose n x n matrix sd_lens_counts keeps (2 GiB)


def _kappa(kappa):
    kappa = float(kappa)
    if not -1.0 <= kappa <= 1.0:
        raise ValueError(f"kappa = 2 / beta - 1 must lie in [-1, 1], got {kappa!r}")
    return kappa


def lens_workspace_bytes(T, n, curve_major=False, m=None):
    """(recommended, floor) workspace sizes of sd_lens_counts and sd_lens_external_counts for a T x n matrix and m targets
    (default: all n): the n x n matrix of squared distances (8 n^2 bytes) and the rows of a batch of whole blocks of 128
    external targets (8 n bytes a target), behind the time-major copy of a curve-major matrix.  The floor holds one block;
    the recommended size holds all targets, up to 1 GiB of rows.  (0, 0) where T < 1, n < 2, n > 16 384 or m < 0."""
    return _curve_sizes("lens", T, n, None, curve_major, m)


def lens_targets_per_batch(T, n, ws_bytes, curve_major=False, m=None):
    """External targets a batch of sd_lens_external_counts takes with ws_bytes of workspace; 0 below the floor.  (Sample
    targets read their rows from the matrix and go in one batch.)"""
    return _curve_per_batch("lens", "targets", T, n, ws_bytes, None, curve_major, m)


def lens_counts(X, kappa, targets=None, device=None, ws_bytes=None, algo=0):
    """int64[m]: G of the lens (kappa = 0), spherical (kappa = 1) or beta-skeleton depth (kappa = 2 / beta - 1) per target
    (sd_lens_counts) -- the pairs i < j of the n columns of X with a + kappa b <= c and b + kappa a <= c, where a, b are
    curve_sqdist's D2 of the target to curves i, j and c that of the two curves, every product and sum rounded on its own.
    The depth is G / C(n, 2).  A target's own pairs count.  algo: 0 takes the form that kappa names, 1 the general form (the
    same integers).  targets, ws_bytes and the contract on X as for curve_sqdist; n is at most 16 384."""
    return _curves("sd_lens_counts", "lens", None, X, targets, device, (_kappa(kappa), int(algo)), ws_bytes,
                   lambda t, dev, M, m: [t.empty((m,), dtype=t.int64, device=dev)])[0]


def lens_external_counts(X, Q, kappa, device=None, ws_bytes=None, algo=0):
    """int64[m]: the counts of lens_counts for the m columns of Q (T x m) against the pairs of the n columns of X
    (sd_lens_external_counts).  The depth is G / C(n, 2) here too.  A column of Q equal to a sample curve gives that curve's
    count."""
    return _external_curves(_lib().sd_lens_external_counts, X, Q, device, _kappa(kappa), int(algo), ws_bytes=ws_bytes,
                            family="lens", outputs=lambda t, dev, T, n, m: [t.empty((m,), dtype=t.int64, device=dev)])[0]


def central_regions_row_capacity():
    """The most curves of the row-resident route of sd_central_regions (whole rows in one workgroup's registers); above
    it the call goes through column blocks.  (torch first, as in _lib: a test may ask this before any device call.)"""
    torch()
    return int(_native.load().sd_central_regions_row_capacity())


def central_regions_workspace_bytes(T, n, L, curve_major=False):
    """The workspace sd_central_regions needs for a T x n matrix and L levels: a fence (16 T bytes), the counts (8 n) and,
    above the row capacity, the column blocks' min / max; 0 for a shape or L the call refuses.  curve_major: the matrix is
    F-contiguous and takes a time-major copy (8 T n) as well."""
    torch()
    lib = _native.load()
    T, n = int(T), int(n)
    return int(lib.sd_central_regions_workspace_bytes(T, n, *_strides(T, n, curve_major), int(L)))


def central_regions(X, level, L=None, box=None, factor=1.5, whiskers=True, device=None, outside=True, fence=True):
    """(env, fence, outside, whisker) of the functional boxplot (sd_central_regions); the entries not asked for are None.
    X: T x n, NaN-free (the depth layer checks; this function takes its array as it is).  level: n bytes in 0 .. L, region l
    = { i : level[i] <= l }, a level >= L in no region.  L: the number of regions (default: min(8, max(level) + 1), so that every
    level present names a region).
    env: float64 [L, 2, T], min and max of every region per timepoint.  box=None: envelopes only.  box in [0, L): fence
    float64 [2, T] = lower - factor * (upper - lower), upper + factor * (upper - lower) of region `box`; outside int32
    [n, 2], the timepoints at which a curve lies below / above the fence; whisker float64 [2, T], min and max over the
    curves with no such timepoint.  whiskers=False, outside=False, fence=False leave the output out (whiskers without
    outside keep the counts on the device); the others do not change."""
    t = torch()
    lv = np.ascontiguousarray(np.asarray(level, dtype=np.uint8))
    if lv.ndim != 1 or lv.shape[0] != np.shape(X)[1]:
        raise ValueError("level must hold one byte per curve")
    L = min(8, int(lv.max()) + 1) if L is None else int(L)
    if not 1 <= L <= 8:
        raise ValueError(f"L must be in [1, 8], got {L}")
    b = -1 if box is None else int(box)
    if not (box is None or 0 <= b < L):
        raise ValueError("box must be None (envelopes only) or the index of a region")
    if not (np.isfinite(factor) and factor >= 0):
        raise ValueError("the fence factor must be finite and not negative")
    lib = _lib()
    M = to_device_matrix(X, device)
    dev = M.device
    lvd = t.from_numpy(lv).to(dev)
    fenced = b >= 0
    env = t.empty((L, 2, M.T), dtype=t.float64, device=dev)
    fen = t.empty((2, M.T), dtype=t.float64, device=dev) if fenced and fence else None
    cnt = t.empty((M.n, 2), dtype=t.int32, device=dev) if fenced and outside else None
    whi = t.empty((2, M.T), dtype=t.float64, device=dev) if fenced and whiskers else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    _launch(dev, lib.sd_central_regions, env, M.tensor.data_ptr(), M.T, M.n, M.st, M.sn, lvd.data_ptr(), L, b, float(factor),
            _OUT, ptr(fen), ptr(cnt), ptr(whi),
            workspace=lambda: _sized(dev, lib.sd_central_regions_workspace_bytes(M.T, M.n, M.st, M.sn, L)), return_tensor=True)
    return tuple(x.cpu().numpy() if x is not None else None for x in (env, fen, cnt, whi))


# Point clouds.  Every depth of K4, K5, K7, K10, K11, K12 and K13 is asked for in three forms ("Point clouds: the three
# forms"): row targets[q] of P inside P, the external point Q[q] inside P u {Q[q]}, the last member of block q inside the
# block.  The public functions below name the C entry point and the form; _points does the rest.
_ROWS, _EXTERNAL, _BLOCKS = "rows", "external", "blocks"


def _points(name, dtype, P, device, form, arg, *extra, U=None, plane=False, workspace=None):
    """lib.<name>(P, n, [d, [U, k,]] selection, *extra, out, [ws, ws_bytes,] stream); out: one value of dtype per target.
    selection: (targets, m) for the rows targets=arg of P (None: all), (Q, m) for the external points Q=arg, or
    (members, nb, bs) for the blocks members=arg (-1 padded at the end, others first, target last).  U: the k x d
    directions of K10 and K12.  plane: K11 and K13 -- P and Q are checked to be planar and exact, d is not passed, and an index outside the
    sample is a ValueError like K11's other argument checks.  workspace(dev, n, d): (buffer, bytes).
    `keep` holds the selection's device tensor until the launch has been issued."""
    assert form in (_ROWS, _EXTERNAL, _BLOCKS)
    t = torch()
    lib = _lib()
    dev = _device(device)
    shape = np.shape(P)
    if len(shape) != 2:
        raise ValueError("expected a 2-D array")
    n = shape[0]
    # the indices first: what would read outside the sample is refused before anything is uploaded
    try:
        if form == _ROWS:
            keep, m, ptr = _targets_dev(arg, n, dev)
            sel = (ptr, m)
        elif form == _BLOCKS:
            keep, m, bs = _members_dev(arg, dev, n, trailing_padding=True)
            sel = (keep.data_ptr(), m, bs)
    except IndexError as e:
        if plane:
            raise ValueError(str(e)) from e
        raise
    Pd = _plane_points(P, dev) if plane else _upload(P, 2, dev)
    d = Pd.shape[1]
    head = (Pd.data_ptr(), n) if plane else (Pd.data_ptr(), n, d)
    if U is not None:
        Ud = _directions_dev(U, d, dev)
        head += (Ud.data_ptr(), Ud.shape[0])
    if form == _EXTERNAL:
        keep = _plane_points(arg, dev, "Q") if plane else _upload(arg, 2, dev)
        if keep.shape[1] != d:
            raise ValueError("Q must have the same number of coordinates as P")
        m = keep.shape[0]
        sel = (keep.data_ptr(), m)
    out = t.empty(m, dtype=dtype, device=dev)
    ws = (lambda: workspace(dev, n, d)) if workspace is not None else None
    return _launch(dev, getattr(lib, name), out, *head, *sel, *extra, workspace=ws)


def l1_depth(P, targets=None, device=None):
    return _points("sd_l1_depth", torch().float64, P, device, _ROWS, targets)


def _simplex_sampled_ws(dev, n, T, d, samples, ws_bytes):
    """(buffer, bytes) of the sampled estimators' workspace: what sd_simplex_sampled_workspace_bytes recommends, or ws_bytes
    (0: no workspace at all, a null pointer)."""
    if ws_bytes is None:
        return _sized(dev, _lib().sd_simplex_sampled_workspace_bytes(n, T, d, int(samples)))
    return _sized(dev, ws_bytes) if ws_bytes else (None, 0)


def pointcloud_simplex_counts(P, targets=None, tol=1e-7, samples=None, seed=0, device=None, ws_bytes=None):
    """ws_bytes: the workspace size a sampled call runs with (default: the recommended one); the counts do not depend on it."""
    if samples is None:
        return _points("sd_pointcloud_simplex_counts", torch().int64, P, device, _ROWS, targets, tol)
    return _points("sd_pointcloud_simplex_sampled", torch().int64, P, device, _ROWS, targets, tol, int(samples), int(seed),
                   workspace=lambda dev, n, d: _simplex_sampled_ws(dev, n, 0, d, samples, ws_bytes))


def multi_simplex_counts(P, targets=None, relax=True, tol=1e-7, samples=None, seed=0, device=None, ws_bytes=None):
    """P: (n, T, d) curves.  ws_bytes as for pointcloud_simplex_counts."""
    t = torch()
    lib = _lib()
    dev = _device(device)
    Pd = _upload(P, 3, dev)
    n, T, d = Pd.shape
    td, m, tp = _targets_dev(targets, n, dev)
    out = t.empty(m, dtype=t.int64, device=dev)
    if samples is None:
        return _launch(dev, lib.sd_multi_simplex_counts, out, Pd.data_ptr(), n, T, d, tp, m, int(bool(relax)), tol)
    return _launch(dev, lib.sd_multi_simplex_sampled, out, Pd.data_ptr(), n, T, d, tp, m, int(bool(relax)), tol,
                   int(samples), int(seed),
                   workspace=lambda: _simplex_sampled_ws(dev, n, T, d, samples, ws_bytes))


def pointcloud_simplex_external_counts(P, Q, tol=1e-7, device=None):
    """int64[m]: (d+1)-subsets of ALL rows of P whose simplex contains the external point Q[q]."""
    return _points("sd_pointcloud_simplex_external_counts", torch().int64, P, device, _EXTERNAL, Q, tol)


def pointcloud_simplex_subset_counts(P, members, tol=1e-7, device=None):
    """int64[nb]: per block (rows of `members`, -1 padded, others first, target last) the (d+1)-subsets of the
    block's others whose simplex contains its target."""
    return _points("sd_pointcloud_simplex_subset_counts", torch().int64, P, device, _BLOCKS, members, tol)


def l1_external_depth(P, Q, device=None):
    """float64[m]: L1 depth of the external point Q[q] inside P u {Q[q]}."""
    return _points("sd_l1_external_depth", torch().float64, P, device, _EXTERNAL, Q)


def l1_subset_depth(P, members, device=None):
    """float64[nb]: L1 depth of each block's target (last row of the block) inside the block."""
    return _points("sd_l1_subset_depth", torch().float64, P, device, _BLOCKS, members)


def oja_volume_sums(P, targets=None, device=None):
    """float64[m]: sum over d-subsets S of the other rows of vol(conv(S u {P[target]})) (sd_oja_volume_sums)."""
    return _points("sd_oja_volume_sums", torch().float64, P, device, _ROWS, targets)


def oja_external_volume_sums(P, Q, device=None):
    """float64[m]: sum over d-subsets S of ALL rows of P of vol(conv(S u {Q[q]})) (sd_oja_external_volume_sums)."""
    return _points("sd_oja_external_volume_sums", torch().float64, P, device, _EXTERNAL, Q)


def oja_subset_volume_sums(P, members, device=None):
    """float64[nb]: per block (rows of `members`, -1 padded, others first, target last) the sum over d-subsets S of
    the block's others of vol(conv(S u {target}))."""
    return _points("sd_oja_subset_volume_sums", torch().float64, P, device, _BLOCKS, members)


def prob_normal_sums(mu, sigma, targets=None, device=None):
    """float64[m]: the reference's normal-depth pair sums, unnormalised (sd_prob_normal_sums): for k = targets[q], the sum
    over pairs i < j of the other distributions of int (Phi_i - Phi_k Phi_j) phi_k.  depth = sums / C(n, 2)."""
    t = torch()
    lib = _lib()
    dev = _device(device)
    mud, sgd = _upload(mu, 1, dev), _upload(sigma, 1, dev)
    n = mud.shape[0]
    if sgd.shape[0] != n:
        raise ValueError("mu and sigma must have the same length")
    td, m, tp = _targets_dev(targets, n, dev)
    out = t.empty(m, dtype=t.float64, device=dev)
    return _launch(dev, lib.sd_prob_normal_sums, out, mud.data_ptr(), sgd.data_ptr(), n, tp, m)


def prob_poisson_sums(lam, lim, targets=None, device=None):
    """float64[m]: the reference's Poisson-depth sums, unnormalised (sd_prob_poisson_sums).  lam: T x n rates (rows are
    timepoints, columns curves); for f = targets[q], the sum over rows t, z = 1 .. lim - 1 and column pairs i < j other
    than f of P(X_f = z) P(X_i <= z) P(X_j >= z).  depth = sums / C(T, 2)."""
    t = torch()
    lib = _lib()
    dev = _device(device)
    Ld = _upload(lam, 2, dev)
    T, n = Ld.shape
    td, m, tp = _targets_dev(targets, n, dev)
    out = t.empty(m, dtype=t.float64, device=dev)
    return _launch(dev, lib.sd_prob_poisson_sums, out, Ld.data_ptr(), T, n, int(lim), tp, m)


def prob_band_sums(mu, var, relax, targets=None, members=None, device=None):
    """float64[m]: band sums of curves under Gaussian noise, unnormalised (sd_prob_band_sums).  mu, var: T x n (rows are
    timepoints, columns curves; X_c(t) ~ N(mu[t, c], var[t, c]) independent, var = 0 a point mass).  For i = targets[q]
    and the pairs j < k of its others -- every other column, or members[q] (-1 padded; the target skipped where listed) --
    the sum over pairs of sum_t p (relax) or prod_t p, p = P(min(X_j, X_k) <= X_i <= max(X_j, X_k)).
    depth = sums / T / C(n', 2) (relax) or sums / C(n', 2), n' counting the target."""
    t = torch()
    shape = np.shape(mu)
    if len(shape) != 2 or tuple(np.shape(var)) != tuple(shape):
        raise ValueError("mu and var must be T x n arrays of the same shape")
    T, n = shape
    lib = _lib()
    dev = _device(device)
    # the indices first: out-of-range ones are refused before mu and var are uploaded
    td, m, tp = _targets_dev(targets, n, dev)
    md, _, bs = _members_dev(members, dev, n, rows=m) if members is not None else (None, 0, 0)
    mud, vd = _upload(mu, 2, dev), _upload(var, 2, dev)
    out = t.empty(m, dtype=t.float64, device=dev)
    return _launch(dev, lib.sd_prob_band_sums, out, mud.data_ptr(), vd.data_ptr(), T, n, tp, m,
                   md.data_ptr() if md is not None else None, bs, int(bool(relax)))


def multi_band_counts(P, targets=None, device=None):
    """int64[m]: sum_t #{pairs of other curves whose componentwise band contains the target at t} (sd_multi_band_counts).
    P: (n, T, d) curves, NaN-free."""
    t = torch()
    lib = _lib()
    dev = _device(device)
    Pd = _upload(P, 3, dev)
    n, T, d = Pd.shape
    if bool(t.isnan(Pd).any()):
        raise ValueError("componentwise band containment ('r2_enum') does not accept NaN values")
    td, m, tp = _targets_dev(targets, n, dev)
    out = t.empty(m, dtype=t.int64, device=dev)
    return _launch(dev, lib.sd_multi_band_counts, out, Pd.data_ptr(), n, T, d, tp, m,
                   workspace=lambda: _sized(dev, lib.sd_multi_band_workspace_bytes(n, T, d)))


def multi_band_j_counts(P, targets=None, J=3, device=None):
    """int64[m, J-1]: column j-2 = sum_t #{j-subsets of the other curves whose componentwise band contains the target at
    t}, j = 2 .. J, J in [2, 4] (sd_multi_band_j_counts).  P: (n, T, d) curves, NaN-free."""
    t = torch()
    lib = _lib()
    dev = _device(device)
    Pd = _upload(P, 3, dev)
    n, T, d = Pd.shape
    if bool(t.isnan(Pd).any()):
        raise ValueError("componentwise band containment ('r2_enum') does not accept NaN values")
    td, m, tp = _targets_dev(targets, n, dev)
    J = int(J)
    out = t.empty((m, max(J - 1, 1)), dtype=t.int64, device=dev)
    return _launch(dev, lib.sd_multi_band_j_counts, out, Pd.data_ptr(), n, T, d, tp, m, J,
                   workspace=lambda: _sized(dev, lib.sd_multi_band_workspace_bytes(n, T, d)))


def _directions_dev(U, d, dev):
    """The k x d direction array on dev (k >= 1 rows of d coordinates)."""
    Ud = _upload(U, 2, dev)
    if Ud.shape[0] < 1 or Ud.shape[1] != d:
        raise ValueError(f"directions must be a k x {d} array with k >= 1")
    return Ud


MULTI_CLOUD_ALGOS = {"auto": 0, "lds": 1, "global": 2}


def _multi_cloud_algo(algo):
    if isinstance(algo, str) and algo not in MULTI_CLOUD_ALGOS:
        raise ValueError(f"algo must be one of {sorted(MULTI_CLOUD_ALGOS)}, got {algo!r}")
    return MULTI_CLOUD_ALGOS[algo] if isinstance(algo, str) else int(algo)


def multi_cloud_lds_capacity():
    """The most curves of the LDS route of sd_multi_halfspace_sums / sd_multi_projection_sums (a cloud's projections sorted
    in one workgroup's LDS); above it 'auto' takes the global route.  (torch first, as in _lib.)"""
    torch()
    return int(_native.load().sd_multi_cloud_lds_capacity())


def _multi_cloud_workspace_bytes(family, n, T, d, k, m, algo):
    lib = _native.load()
    n, T, d, k, a = int(n), int(T), int(d), int(k), _multi_cloud_algo(algo)
    m = n if m is None else int(m)
    return (int(getattr(lib, f"sd_multi_{family}_workspace_bytes")(n, T, d, k, m, a)),
            int(getattr(lib, f"sd_multi_{family}_min_workspace_bytes")(n, T, d, k, m, a)))


def multi_halfspace_workspace_bytes(n, T, d, k, m=None, algo="auto"):
    """(recommended, floor) workspace sizes of sd_multi_halfspace_sums for n curves x T timepoints x d features, k directions
    and m targets (default: all n); the floor holds one timepoint per batch.  (0, 0) for a shape or algo the call refuses."""
    return _multi_cloud_workspace_bytes("halfspace", n, T, d, k, m, algo)


def multi_projection_workspace_bytes(n, T, d, k, m=None, algo="auto"):
    """(recommended, floor) workspace sizes of sd_multi_projection_sums; as multi_halfspace_workspace_bytes."""
    return _multi_cloud_workspace_bytes("projection", n, T, d, k, m, algo)


def _multi_cloud_sums(family, dtype, P, U, targets, device, algo, ws_bytes):
    t = torch()
    lib = _lib()
    dev = _device(device)
    a = _multi_cloud_algo(algo)
    shape = np.shape(P)
    if len(shape) != 3:
        raise ValueError("expected a 3-D array (curves x timepoints x features)")
    n, T, d = shape
    td, m, tp = _targets_dev(targets, n, dev)                        # the indices first: refused before anything is uploaded
    Pd = _upload(P, 3, dev)
    Ud = _directions_dev(U, d, dev)
    k = Ud.shape[0]
    out = t.empty((m, 2), dtype=dtype, device=dev)
    size = getattr(lib, f"sd_multi_{family}_workspace_bytes")
    return _launch(dev, getattr(lib, f"sd_multi_{family}_sums"), out, Pd.data_ptr(), n, T, d, Ud.data_ptr(), k, tp, m, a,
                   workspace=lambda: _sized(dev, size(n, T, d, k, m, a) if ws_bytes is None else ws_bytes))


def multi_halfspace_sums(P, U, targets=None, device=None, algo="auto", ws_bytes=None):
    """int64[m, 2]: the records (SH, MH) of the halfspace depth of multivariate curves over time (sd_multi_halfspace_sums).
    P: (n, T, d) curves, U: k x d directions shared by all timepoints.  With h_t the halfspace count of the curve's point
    inside the cloud of all curves' points at t (halfspace_counts on P[:, t, :]): SH = sum_t h_t, MH = min_t h_t; the mean
    depth is SH / (n T), the infimal depth MH / n.  P must be finite (the depth layer checks; this function takes its array
    as it is).  algo: 'auto', 'lds' (n <= multi_cloud_lds_capacity()) or 'global', or their numbers 0, 1, 2.  ws_bytes: the
    workspace size to run with (default: the recommended one); the records do not depend on it or on algo, below the floor
    the library refuses."""
    return _multi_cloud_sums("halfspace", torch().int64, P, U, targets, device, algo, ws_bytes)


def multi_projection_sums(P, U, targets=None, device=None, algo="auto", ws_bytes=None):
    """float64[m, 2]: the records (PS, OM) of the projection depth of multivariate curves over time
    (sd_multi_projection_sums).  With O_t the Stahel-Donoho outlyingness of the curve's point inside the cloud at t
    (projection_outlyingness on P[:, t, :]): PS = sum_t 1 / (1 + O_t), added in ascending t (the last entry of np.cumsum),
    OM = max_t O_t; the mean depth is PS / T, the infimal depth 1 / (1 + OM).  P and U: finite, magnitudes of at most 2^500
    (projection_check; the depth layer checks).  algo and ws_bytes as for multi_halfspace_sums; the same bits whatever
    they are."""
    return _multi_cloud_sums("projection", torch().float64, P, U, targets, device, algo, ws_bytes)


def multi_outlyingness_workspace_bytes(n, T, d, k, m=None, algo="auto"):
    """(recommended, floor) workspace sizes of sd_multi_outlyingness_moments: multi_projection_workspace_bytes' plus the
    centres of a batch's timepoints."""
    return _multi_cloud_workspace_bytes("outlyingness", n, T, d, k, m, algo)


def multi_outlyingness_moments(P, U, targets=None, device=None, algo="auto", ws_bytes=None, centres=False, curves=False):
    """float64[m, d + 1]: the Welford records (M_0 .. M_(d-1), Q) of the directional outlyingness of multivariate curves
    (sd_multi_outlyingness_moments; Dai & Genton).  P: (n, T, d) curves, U: k x d directions.  Per timepoint the
    Stahel-Donoho outlyingness o_t of multi_projection_sums is given the direction of the unit vector from the cloud's
    deepest point c_t (the lowest index among the minimisers of o_t over all n curves) to the curve's point:
    O_t = o_t (x - x_c) / |x - x_c|, the zero vector where |x - x_c| = 0; M is the running mean of O_t over ascending t
    and Q the running sum of squared deviations (Welford).  MO = M, VO = Q / T, FO = |MO|^2 + VO.  Where a direction's MAD
    is 0 at some timepoint a record is +-inf or NaN (IEEE, not special-cased).  centres=True adds the int64[T] array c_t,
    curves=True the float64[m, T, d] array O_t to the result (a tuple in that order).  With an empty target list nothing
    is launched and the library writes no centres: they come back as an empty array, not as T zeros that would read as
    curve 0.  P and U: finite, magnitudes of at most 2^500 (projection_check, run here, so that the function is safe on
    its own: it also keeps the sum of squared differences from overflowing.  DirectionalOutlyingness has checked already;
    the second host pass over P is small against the call).  algo and
    ws_bytes as for multi_halfspace_sums; the same bits whatever they are."""
    t = torch()
    lib = _lib()
    dev = _device(device)
    a = _multi_cloud_algo(algo)
    shape = np.shape(P)
    if len(shape) != 3:
        raise ValueError("expected a 3-D array (curves x timepoints x features)")
    n, T, d = shape
    for what, A in (("coordinates", P), ("direction entries", U)):  # (a tensor comes to the host for it)
        projection_check(what, A.detach().cpu().numpy() if isinstance(A, t.Tensor) else A)
    td, m, tp = _targets_dev(targets, n, dev)                        # the indices first: refused before anything is uploaded
    Pd = _upload(P, 3, dev)
    Ud = _directions_dev(U, d, dev)
    k = Ud.shape[0]
    out = t.empty((m, d + 1), dtype=t.float64, device=dev)
    cen = t.empty(T if m else 0, dtype=t.int64, device=dev) if centres else None   # (no targets: nothing is launched)
    cur = t.empty((m, T, d), dtype=t.float64, device=dev) if curves else None
    rec = _launch(dev, lib.sd_multi_outlyingness_moments, out, Pd.data_ptr(), n, T, d, Ud.data_ptr(), k, tp, m, a, _OUT,
                  cen.data_ptr() if centres else None, cur.data_ptr() if curves else None,
                  workspace=lambda: _sized(dev, lib.sd_multi_outlyingness_workspace_bytes(n, T, d, k, m, a)
                                           if ws_bytes is None else ws_bytes))
    if not centres and not curves:
        return rec
    return (rec,) + ((cen.cpu().numpy(),) if centres else ()) + ((cur.cpu().numpy(),) if curves else ())


def halfspace_workspace_bytes(n, d, k):
    """(recommended, floor) workspace sizes of sd_halfspace_counts; the floor holds one direction per chunk."""
    lib = _native.load()
    return (int(lib.sd_halfspace_workspace_bytes(int(n), int(d), int(k))),
            int(lib.sd_halfspace_min_workspace_bytes(int(n), int(d), int(k))))


def halfspace_counts(P, U, targets=None, device=None, workspace_budget=None, algo="rank"):
    """int64[m]: min over the rows u of U (k x d) of min(#{i: p_i.u <= x.u}, #{i: p_i.u >= x.u}) for x = P[targets[q]], the
    target and every tie counted (sd_halfspace_counts); depth = counts / n.  workspace_budget: upper bound in bytes for
    the scratch buffer (default: the recommended size), never below the floor of one direction per chunk; the counts do
    not depend on it.  algo='pairwise': the same counts from the pairwise kernel (sd_halfspace_pairwise_counts)."""
    if algo == "pairwise":
        return _points("sd_halfspace_pairwise_counts", torch().int64, P, device, _ROWS, targets, U=U)
    if algo != "rank":
        raise ValueError("algo must be 'rank' or 'pairwise'")

    def sized(dev, n, d):
        want, floor = halfspace_workspace_bytes(n, d, np.shape(U)[0])
        if workspace_budget is not None:
            want = max(floor, min(want, int(workspace_budget)))
        return _sized(dev, want)
    return _points("sd_halfspace_counts", torch().int64, P, device, _ROWS, targets, U=U, workspace=sized)


def halfspace_external_counts(P, Q, U, device=None):
    """int64[m]: the halfspace counts of the external point Q[q] inside P u {Q[q]} (n + 1 points, Q[q] counted once) over
    the directions U (sd_halfspace_external_counts); depth = counts / (n + 1)."""
    return _points("sd_halfspace_external_counts", torch().int64, P, device, _EXTERNAL, Q, U=U)


def halfspace_subset_counts(P, members, U, device=None):
    """int64[nb]: per block (rows of `members`, -1 padded, target last) the halfspace counts of the block's target inside
    the block over the directions U (sd_halfspace_subset_counts); depth = counts / block size."""
    return _points("sd_halfspace_subset_counts", torch().int64, P, device, _BLOCKS, members, U=U)


HALFSPACE2_ALGOS = {"auto": 0, "sweep": 1, "pairwise": 2}
_HALFSPACE2_MAX_ABS = 2.0 ** 500


def _halfspace2_algo(algo):
    if algo not in HALFSPACE2_ALGOS:
        raise ValueError("algo must be 'auto', 'sweep' or 'pairwise'")
    return HALFSPACE2_ALGOS[algo]


def _plane_points(A, dev, what="P"):
    """The n x 2 point array on dev: finite, |coordinate| <= 2^500 (the exact predicate's products must not overflow)."""
    t = torch()
    Ad = _upload(A, 2, dev)
    if Ad.shape[1] != 2:
        raise ValueError(f"exact halfspace and simplicial counts are defined for points in the plane: {what} must be n x 2")
    if Ad.numel() and not bool((Ad.abs() <= _HALFSPACE2_MAX_ABS).all()):      # NaN fails the comparison too
        raise ValueError("the exact predicate needs finite coordinates of magnitude at most 2^500")
    return Ad


def halfspace_exact_counts(P, targets=None, device=None, algo="auto"):
    """int64[m]: the exact halfspace (Tukey) counts of x = P[targets[q]] inside the planar sample P (n x 2): the fewest
    sample points in a closed halfplane with x on its boundary, x and its duplicates counted (sd_halfspace2_counts);
    depth = counts / n.  algo: 'auto', 'sweep' (samples of at most 8192 points) or 'pairwise'; the same integers."""
    return _points("sd_halfspace2_counts", torch().int64, P, device, _ROWS, targets, _halfspace2_algo(algo), plane=True)


def halfspace_exact_external_counts(P, Q, device=None, algo="auto"):
    """int64[m]: the exact halfspace counts of the external point Q[q] inside P u {Q[q]} (n + 1 points, Q[q] counted once;
    sd_halfspace2_external_counts); depth = counts / (n + 1)."""
    return _points("sd_halfspace2_external_counts", torch().int64, P, device, _EXTERNAL, Q, _halfspace2_algo(algo), plane=True)


def halfspace_exact_subset_counts(P, members, device=None, algo="auto"):
    """int64[nb]: per block (rows of `members`, -1 padded, target last) the exact halfspace counts of the block's target
    inside the block (sd_halfspace2_subset_counts); depth = counts / block size."""
    return _points("sd_halfspace2_subset_counts", torch().int64, P, device, _BLOCKS, members, _halfspace2_algo(algo), plane=True)


def simplicial_exact_counts(P, targets=None, device=None, algo="auto"):
    """int64[m]: the exact simplicial counts of x = P[targets[q]] inside the planar sample P (n x 2): the triples of the
    other n - 1 rows whose closed triangle contains x, decided with exact signs (sd_simplicial2_counts); depth = counts /
    C(n, 3).  algo: 'auto', 'sweep' (at most 8192 others) or 'pairwise'; the same integers."""
    return _points("sd_simplicial2_counts", torch().int64, P, device, _ROWS, targets, _halfspace2_algo(algo), plane=True)


def simplicial_exact_external_counts(P, Q, device=None, algo="auto"):
    """int64[m]: the triples of ALL n rows of P whose closed triangle contains the external point Q[q]
    (sd_simplicial2_external_counts); depth = counts / C(n + 1, 3)."""
    return _points("sd_simplicial2_external_counts", torch().int64, P, device, _EXTERNAL, Q, _halfspace2_algo(algo), plane=True)


def simplicial_exact_subset_counts(P, members, device=None, algo="auto"):
    """int64[nb]: per block (rows of `members`, -1 padded, others first, target last) the triples of the block's others whose
    closed triangle contains its target (sd_simplicial2_subset_counts); depth = counts / C(block size, 3)."""
    return _points("sd_simplicial2_subset_counts", torch().int64, P, device, _BLOCKS, members, _halfspace2_algo(algo), plane=True)


_PROJECTION_MAX_ABS = 2.0 ** 500


def projection_workspace_bytes(n, d, k):
    """(recommended, floor) workspace sizes of sd_projection_outlyingness and sd_projection_external_outlyingness; the
    floor holds one direction per chunk."""
    lib = _native.load()
    return (int(lib.sd_projection_workspace_bytes(int(n), int(d), int(k))),
            int(lib.sd_projection_min_workspace_bytes(int(n), int(d), int(k))))


def projection_check(what, *arrays):
    """The value check of projection depth, in one place: every entry finite with magnitude at most 2^500, so that no
    projection, midpoint or deviation overflows and no NaN arises (NaN fails the comparison too).  The callers that
    take user data (PointcloudDepth, PointcloudHomogeneity) run it once, on the host, before anything else; the
    projection_* functions below do not repeat it -- like halfspace_counts they take their arrays as they are."""
    for A in arrays:
        A = np.asarray(A, dtype=np.float64)
        if A.size and not bool((np.abs(A) <= _PROJECTION_MAX_ABS).all()):
            raise ValueError(f"projection depth needs finite {what} of magnitude at most 2^500")


def _projection_workspace(U, workspace_budget):
    def sized(dev, n, d):
        want, floor = projection_workspace_bytes(n, d, np.shape(U)[0])
        if workspace_budget is not None:
            want = max(floor, min(want, int(workspace_budget)))
        return _sized(dev, want)
    return sized


def projection_outlyingness(P, U, targets=None, device=None, workspace_budget=None):
    """float64[m]: the Stahel-Donoho outlyingness max over the rows u of U (k x d) of |x.u - med(P.u)| / MAD(P.u) for
    x = P[targets[q]] inside the sample P (sd_projection_outlyingness; DESIGN §3 K12 states every rounding);
    depth = 1 / (1 + outlyingness).  +inf where a direction has MAD 0 and x is off its median.  workspace_budget: upper
    bound in bytes for the scratch buffer (default: the recommended size), never below the floor of one direction per
    chunk; the result does not depend on it.  P and U: finite, magnitudes of at most 2^500, no all-zero direction
    (projection_check; the public API checks)."""
    return _points("sd_projection_outlyingness", torch().float64, P, device, _ROWS, targets, U=U,
                   workspace=_projection_workspace(U, workspace_budget))


def projection_external_outlyingness(P, Q, U, device=None, workspace_budget=None):
    """float64[m]: the outlyingness of the external point Q[q] inside P u {Q[q]} (n + 1 points: a median and a MAD per
    external point and direction; sd_projection_external_outlyingness)."""
    return _points("sd_projection_external_outlyingness", torch().float64, P, device, _EXTERNAL, Q, U=U,
                   workspace=_projection_workspace(U, workspace_budget))


def projection_subset_outlyingness(P, members, U, device=None):
    """float64[nb]: per block (rows of `members`, -1 padded, target last; at most 2048 members) the outlyingness of the
    block's target inside the block (sd_projection_subset_outlyingness); an empty block gives 0."""
    return _points("sd_projection_subset_outlyingness", torch().float64, P, device, _BLOCKS, members, U=U)


# ---- K23: projections of curves on a direction set, and the random projection depths (statdepth_hip_projections.h) ----
def _projected_size(name, T, n, k, curve_major, *more):
    """sd_<name>(T, n, st, sn, k, *more)."""
    T, n = int(T), int(n)
    return int(getattr(_native.load(), f"sd_{name}")(T, n, *_strides(T, n, curve_major), int(k), *more))


def curve_projections_workspace_bytes(T, n, k, curve_major=False):
    """(recommended, floor) workspace sizes of sd_curve_projections: it needs none, both are 0."""
    size = _projected_size("curve_projections_workspace_bytes", T, n, k, curve_major)
    return size, size


def rp_depth_workspace_bytes(T, n, k, algo="auto", curve_major=False, m=None):
    """(recommended, floor) workspace sizes of sd_rp_depth_sums for T x n curves and k directions: a chunk of rows of the
    k x n projections and K14's need for it -- all k rows at the recommended size while they are within 1 GiB, one row at the
    floor.  Neither layout takes a copy."""
    tail = (int(n if m is None else m), RANK_DEPTH_ALGOS[algo] if isinstance(algo, str) else int(algo))
    return tuple(_projected_size(f"rp_depth_{name}", T, n, k, curve_major, *tail) for name in ("workspace_bytes", "min_workspace_bytes"))


def rp_outlyingness_workspace_bytes(T, n, k, curve_major=False, m=None):
    """(recommended, floor) workspace sizes of sd_rp_outlyingness: about 32 n bytes a direction of a chunk, one direction
    at the floor."""
    tail = (int(n if m is None else m),)
    return tuple(_projected_size(f"rp_outlyingness_{name}", T, n, k, curve_major, *tail)
                 for name in ("workspace_bytes", "min_workspace_bytes"))


def _projected(fn, sizes, X, U, targets, device, own, ws_bytes, output):
    """lib.<fn>(X, T, n, st, sn, U, k, [targets, m,] *own, out, ws, ws_bytes, stream).  targets False: the entry point takes
    none.  sizes(M, k, m): the (recommended, floor) pair; ws_bytes None runs with the recommended size.  output(t, dev, M, k, m):
    the output tensor."""
    t = torch()
    lib = _lib()
    M = to_device_matrix(X, device)
    dev = M.device
    Ud = _directions_dev(U, M.T, dev)
    k = int(Ud.shape[0])
    sel, m = (), M.n
    if targets is not False:
        td, m, tp = _targets_dev(targets, M.n, dev)
        sel = (tp, m)
    out = output(t, dev, M, k, m)

    def workspace():
        size = sizes(M, k, m)[0] if ws_bytes is None else int(ws_bytes)
        return _sized(dev, size) if size else (None, 0)
    return _launch(dev, getattr(lib, fn), out, M.tensor.data_ptr(), M.T, M.n, M.st, M.sn, Ud.data_ptr(), k, *sel, *own,
                   workspace=workspace)


def curve_projections(X, U, device=None):
    """float64[k, n]: Z[r, i] = ((X[0, i] U[r, 0] + X[1, i] U[r, 1]) + X[2, i] U[r, 2]) + ... (sd_curve_projections): the
    projections of the n curves (columns of the T x n matrix X, either memory order) on the k rows of U (k x T), timepoints
    in increasing order, every product and every sum rounded separately to fp64 and the first term the product alone -- the
    bits of the numpy loop `z = X[0] * u[0]; for t in 1 .. T-1: z = z + X[t] * u[t]`."""
    return _projected("sd_curve_projections", lambda M, k, m: curve_projections_workspace_bytes(M.T, M.n, k, M.sn != 1), X, U,
                      False, device, (), None, lambda t, dev, M, k, m: t.empty((k, M.n), dtype=t.float64, device=dev))


def rp_depth_sums(X, U, targets=None, device=None, algo="auto", ws_bytes=None):
    """int64[m, 5]: K14's records (SA, SB, SF, SM, MM) over the k rows of curve_projections(X, U) instead of timepoints
    (sd_rp_depth_sums): per target the sums over the directions of A (other curves projected strictly above), of B (strictly
    below), of |2A - n| and of max(A, B), and the maximum over the directions of max(A, B).  X and U finite (the depth layer
    checks).  algo: 'auto', 'image' (n <= 16 384) or 'sort', or 0, 1, 2.  ws_bytes: the workspace size to run with (default:
    the recommended one); the records do not depend on it, below the floor the library refuses."""
    a = RANK_DEPTH_ALGOS[algo] if isinstance(algo, str) else int(algo)
    return _projected("sd_rp_depth_sums", lambda M, k, m: rp_depth_workspace_bytes(M.T, M.n, k, a, M.sn != 1, m), X, U, targets,
                      device, (a,), ws_bytes, lambda t, dev, M, k, m: t.empty((m, 5), dtype=t.int64, device=dev))


def rp_outlyingness(X, U, targets=None, device=None, ws_bytes=None):
    """float64[m]: max over the rows r of curve_projections(X, U) of |z_r(q) - med_r| / mad_r, K12's median, MAD, division
    and zero cases on every row (sd_rp_outlyingness); depth = 1 / (1 + outlyingness).  +inf where a direction has MAD 0 and
    the target is off its median.  X and U: finite, magnitudes of at most 2^500 (projection_check; the depth layer checks)."""
    return _projected("sd_rp_outlyingness", lambda M, k, m: rp_outlyingness_workspace_bytes(M.T, M.n, k, M.sn != 1, m), X, U,
                      targets, device, (), ws_bytes, lambda t, dev, M, k, m: t.empty((m,), dtype=t.float64, device=dev))
