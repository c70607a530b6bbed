"""The Python side of a PASS HANDLE, once: what Resampler, LogMel, Mp2Encoder and TsProgram (C ABI parts 11, 12, 9, 10) share.
A pass handle's calls are pure enqueues, one pass in flight at a time; sync() or a reader of device results settles it (the
host runtime's half: jsmpeg_amd/csrc/pass_state.h).  Here: the binding of a signature table, the lifecycle as a base class
driven by the handle's symbol prefix, the chained row-shaped outputs of the resampler and the log-mel features, and the
marshalling of a call's streams with the walkers over Mp2Batch and Mp2Live that the resampler and the MP2 encoder share.  A new
pass declares its table and subclasses Pass.  Private: the four modules are the public surface."""
import ctypes

import numpy as np

from . import batch as _batch

END = 1
CHAIN = 2
SAMPLES_PER_FRAME = 1152
DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}
_HOST = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}      # bfloat16 as its bits
_TYPESTR = {"float32": "<f4", "float16": "<f2", "bfloat16": "<i2"}

vp, u32, u64, c_int, i64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_int64
p_u32, p_u64, p_f32 = ctypes.POINTER(u32), ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_float)


def bind(L, table):
    """sets restype / argtypes from {name: (restype, argtypes)}"""
    for name, (res, args) in table.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


_lib = None


def lib():
    """libjsmpeg_hip with jsmpeg_hip_device_read bound: what the four modules bind their tables on"""
    global _lib
    if _lib is None:
        _lib = bind(_batch.lib(), {"jsmpeg_hip_device_read": (c_int, [vp, vp, u64])})
    return _lib


class Pass:
    """create / destroy / sync / query / timings of jsmpeg_hip_<PREFIX>*; a subclass sets PREFIX and calls _open"""
    PREFIX = None
    TIMINGS = ("kernel_ms", "total_ms")

    def _open(self, L, table, cfg):
        """creates the handle; the table's functions of this handle stay bound in _fn under their names behind PREFIX, so that
        a call costs what a call through self.L cost"""
        self.L = L
        self._fn = {name[len(self.PREFIX):]: getattr(L, name) for name in table if name.startswith(self.PREFIX)}
        self.h = self._fn["create"](ctypes.byref(cfg))
        if not self.h:
            raise RuntimeError(self.PREFIX + "create: " + _batch.last_error())

    def _ok(self, rc):
        if rc < 0:
            raise RuntimeError(_batch.last_error())
        return rc

    def _call(self, name, *args):
        """jsmpeg_hip_<PREFIX><name>(handle, ...); a negative answer is raised with the library's message"""
        rc = self._fn[name](self.h, *args)
        if rc < 0:
            raise RuntimeError(_batch.last_error())
        return rc

    def _pair(self, name, *args):
        """... whose last two arguments are uint64 results"""
        a, b = u64(), u64()
        if self._fn[name](self.h, *args, ctypes.byref(a), ctypes.byref(b)) < 0:
            raise RuntimeError(_batch.last_error())
        return int(a.value), int(b.value)

    def _buffer(self, name):
        """(device address, bytes) from the reader that returns the address of the last call's buffer"""
        total = u64()
        p = self._fn[name](self.h, ctypes.byref(total))
        if not p:
            raise RuntimeError(_batch.last_error())
        return p, int(total.value)

    def close(self):
        if self.h:
            self._fn["destroy"](self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._call("sync")

    def query(self):
        """True once the pass in flight has finished on the device; never waits"""
        return bool(self._call("query"))

    def timings(self):
        ms = (ctypes.c_float * 2)()
        self._call("timings", ms)
        return {self.TIMINGS[0]: float(ms[0]), self.TIMINGS[1]: float(ms[1])}


def marshal(ptrs, counts, streams, counts_refusal):
    """a call's streams as the C ABI takes them: (the pointer array, the counts as uint32, the stream numbers as uint32 or
    None, the numbers as a list -- 0, 1, .. without streams)"""
    n = len(ptrs)
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    if cnt.shape != (n,):
        raise ValueError(counts_refusal)
    st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    if st is not None and st.shape != (n,):
        raise ValueError("streams: one stream number per stream")
    arr = (vp * max(1, n))(*[int(p) if p else None for p in ptrs])
    return arr, cnt, st, list(range(n)) if st is None else [int(v) for v in st]


class RowPass(Pass):
    """a chained handle whose last call leaves rows per stream in ONE device buffer (stream_out, out, chain_reset and
    chain_info of three words in its C ABI).  A subclass sets dtype."""

    def _submit(self, name, counts_refusal, ptrs, counts, streams, chain, end, stream):
        arr, cnt, st, numbers = marshal(ptrs, counts, streams, counts_refusal)
        self._call(name, arr, cnt.ctypes.data, None if st is None else st.ctypes.data, len(ptrs), (END if end else 0) | (CHAIN if chain else 0), stream)
        self._numbers = numbers

    def numbers(self):
        """the stream numbers of the last call, in call order"""
        return list(self._numbers)

    def stream_out(self, stream):
        """(offset, count) of stream NUMBER `stream` in the last call's buffer: the element index of its first row (frames
        form: its first frame) and its valid columns (samples per channel, feature frames, whole frames).  Answered without
        waiting."""
        return self._pair("stream_out", stream)

    def counts(self):
        """the count of every stream of the last call, in call order"""
        return [self.stream_out(s)[1] for s in self._numbers]

    def device_out(self):
        """(device address, bytes) of the last call's buffer: closed form, nothing is waited for -- the contents are there for
        work enqueued behind the call on its HIP stream, or after sync()"""
        return self._buffer("out")

    def chain_reset(self, stream=None):
        """ends the chain of `stream` (None: of every stream): its next chained call starts from nothing"""
        self._call("chain_reset", 0xffffffff if stream is None else stream)

    def chain_info(self, stream):
        """(whether `stream` has chain state, the input samples it has taken, the outputs it has made)"""
        out = (u64 * 3)()
        self._call("chain_info", stream, out)
        return bool(out[0]), int(out[1]), int(out[2])

    def _tensor(self, shape):
        """the last call's buffer as a torch tensor of `shape` OVER the device memory; settles the pass"""
        import torch
        self.sync()
        p, total = self.device_out()
        if not shape[0]:
            return torch.empty(shape, dtype=getattr(torch, self.dtype), device="cuda")

        class _Span:
            __cuda_array_interface__ = {"shape": shape, "typestr": _TYPESTR[self.dtype], "data": (p, False), "version": 2}
        assert total == shape[0] * shape[1] * shape[2] * (4 if self.dtype == "float32" else 2)
        t = torch.as_tensor(_Span(), device="cuda")
        return t.view(torch.bfloat16) if self.dtype == "bfloat16" else t

    def _host(self, shape):
        """the last call's buffer on the host in the handle's dtype; shape None: float32 frames [frames][2][1152]"""
        self.sync()
        p, total = self.device_out()
        if shape is None:
            out = np.zeros((total // (2 * SAMPLES_PER_FRAME * 4), 2, SAMPLES_PER_FRAME), np.float32)
        else:
            out = np.zeros(shape, _HOST[self.dtype])
        if total:
            self._ok(self.L.jsmpeg_hip_device_read(out.ctypes.data, p, total))
        return out


# ---------------------------------------------------------------------------------------------------- [frame][2][1152] sources
# what Resampler and Mp2Encoder take besides raw pointers; `who` is the caller's method name, `takes` its wording of the rate

def frames_tensor(x, who):
    """a contiguous float32 CUDA tensor [S, F, 2, 1152] -> (ptrs, frame counts, torch's current stream of its device)"""
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() != 4 or not x.is_contiguous() or \
            tuple(x.shape[2:]) != (2, SAMPLES_PER_FRAME):
        raise ValueError("%s: a contiguous float32 CUDA tensor [S, F, 2, 1152] is needed" % who)
    s, f = int(x.shape[0]), int(x.shape[1])
    step = f * 2 * SAMPLES_PER_FRAME * 4
    return [x.data_ptr() + i * step if f else 0 for i in range(s)], [f] * s, torch.cuda.current_stream(x.device).cuda_stream


def batch_frames(mp2batch, rate, who, takes):
    """every frame of an Mp2Batch's last decode, straight from its PCM in HBM -> (ptrs, frame counts), the batch's streams in
    order; a stream that is not sampled at `rate` is refused"""
    n = mp2batch.n_streams
    counts = [mp2batch.frame_count(s) for s in range(n)]
    for s in range(n):
        if counts[s] and mp2batch.frame_info(s, 0)[2] != rate:
            raise ValueError("%s: stream %d is sampled at %d Hz, %s %d" % (who, s, mp2batch.frame_info(s, 0)[2], takes, rate))
    base, before = mp2batch.pcm_device_pointer(), 0
    ptrs = []
    for c in counts:
        ptrs.append(base + before * 2 * SAMPLES_PER_FRAME * 4)
        before += c
    return ptrs, counts


def live_frames(mp2live, rate, max_streams, chain, who, takes):
    """the frames of an Mp2Live's last tick from their device_pcm pointers (they lie stream after stream, a stream's frames
    contiguous) -> (the frames in that order, ptrs, frame counts, stream numbers).  chain: the live stream id IS the stream
    number (an id at or above max_streams is refused); otherwise numbers is None: 0, 1, .. in the order of the ids"""
    frames = sorted(mp2live.frames(), key=lambda f: f["stream"])
    ids = sorted({f["stream"] for f in frames})
    for f in frames:
        if f["sample_rate"] != rate:
            raise ValueError("%s: stream %d is sampled at %d Hz, %s %d" % (who, f["stream"], f["sample_rate"], takes, rate))
    if chain and ids and ids[-1] >= max_streams:
        raise ValueError("%s: live stream id %d >= max_streams %d" % (who, ids[-1], max_streams))
    ptrs = [next(f["device_pcm"] for f in frames if f["stream"] == i) for i in ids]
    counts = [sum(1 for f in frames if f["stream"] == i) for i in ids]
    return frames, ptrs, counts, ids if chain else None
