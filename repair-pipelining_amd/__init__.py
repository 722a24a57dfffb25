"""repair_pipelining_amd -- MI355X-native GF(256) erasure engine.

Host-side mirror of the reference's coding API (krishnarb3/repair-pipelining:
rs/ ``com.backblaze.erasure``, clay/ ``distributed.erasure.coding.clay``,
lrc/ ``distributed.erasure.coding``) over the C ABI of libecx.so
(include/ecx.h).  Method names, argument meaning and error behaviour follow
the Java classes; byte[] becomes a 1-D ``numpy.uint8`` array and Java
exceptions become :class:`EcxError` carrying the ecx_status code.

All arithmetic runs in hand-written HIP kernels on the MI355X; the host side
only plans (GF tables, matrix inverses, the composed Clay map).  There is no
CPU fallback.

Batch (device-resident) APIs take torch CUDA tensors or raw device pointers.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, Optional, Sequence

import numpy as np

from ._lib import EcxError, build, check, lib, LIB_PATH, HEADER  # noqa: F401

__all__ = [
    "EcxError", "Galois", "Matrix", "CodingLoop", "InputOutputByteTableCodingLoop",
    "InputOutputByteTableCodingLoopSingle", "ReedSolomon", "GfMap", "ClayCodeUtil",
    "ClayCodeErasureDecodingStep", "ClayCode", "LRCErasureCode", "LRCErasureUtil", "JavaRandom",
    "lrc_encode", "lrc_encode_using_single", "lrc_decode", "sample_encode", "sample_decode",
    "device_count", "set_device", "fill_random", "count_mismatch", "shard_stripes",
    "ECChunk", "ECBlock", "ClayCodeHelper", "write_subchunk", "read_subchunk",
    "PatternSet", "index_patterns", "ClayPatternSet", "index_erased", "pair_index", "pair_of",
]


def shard_stripes(n_stripes: int, world: int, rank: int):
    """Stripe range [begin, end) that rank `rank` of `world` owns.  Stripes are
    independent (every repair reads only its own stripe), so the batch is split
    into contiguous ranges with no data exchange between GPUs."""
    if world <= 0 or not 0 <= rank < world or n_stripes < 0:
        raise ValueError("invalid partition request")
    base, extra = divmod(n_stripes, world)
    begin = rank * base + min(rank, extra)
    return begin, begin + base + (1 if rank < extra else 0)


# ---------------------------------------------------------------- ECChunk.java / ECBlock.java
class ECChunk:
    """Hadoop-style chunk wrapper (ECChunk.java:37-109); the buffer may be None."""

    def __init__(self, buffer=None, offset: int = 0, length: Optional[int] = None):
        if buffer is not None and (offset or length is not None):
            buffer = buffer[offset:offset + (len(buffer) - offset if length is None else length)]
        self.buffer = buffer
        self.allZero = False

    def getBuffer(self):
        return self.buffer

    def isAllZero(self):
        return self.allZero

    def setAllZero(self, v: bool):
        self.allZero = v

    def toBytesArray(self) -> np.ndarray:
        return np.array(self.buffer, np.uint8)

    @staticmethod
    def toBuffers(chunks):
        """ECChunk.toBuffers (ECChunk.java:81-95): null chunks map to null buffers."""
        return [None if c is None else c.getBuffer() for c in chunks]


class ECBlock:
    """ECBlock.java:36-99 -- flags are carried but, as in the reference, unused by the math."""

    def __init__(self, chunk: Optional[ECChunk] = None, isParity: bool = False, isErased: bool = False):
        self.chunk, self.isParity, self.isErased = chunk, isParity, isErased

    def getChunk(self):
        return self.chunk

    def setChunk(self, c):
        self.chunk = c


def _buffers(items):
    """Accept ndarray / None / ECChunk / ECBlock entries (the reference passes ECChunk[])."""
    out = []
    for it in items:
        if isinstance(it, ECBlock):
            it = it.chunk
        if isinstance(it, ECChunk):
            it = it.buffer
        out.append(it)
    return out


# ---------------------------------------------------------------- helpers
def _u8(a) -> np.ndarray:
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous):
        raise TypeError("byte buffers must be C-contiguous numpy.uint8 arrays")
    return a


def _addr(a: np.ndarray) -> int:
    """Data address of a checked uint8 array.  ctypes' from_buffer is about 3x cheaper
    than ndarray.ctypes.data (which builds a helper object per call) -- it matters
    for per-call APIs that take 50+ buffers; read-only or empty arrays take the slow
    path."""
    try:
        return ctypes.addressof(ctypes.c_char.from_buffer(a))
    except (TypeError, ValueError):
        return a.ctypes.data


def _ptr_array(bufs) -> ctypes.Array:
    arr = (ctypes.c_void_p * max(1, len(bufs)))()
    arr[:len(bufs)] = [None if b is None else _addr(_u8(b)) for b in bufs]
    return arr


def _bytes(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64) & 0xFF, dtype=np.uint8)


def _dev_ptr(x) -> int:
    """Device pointer of a torch CUDA tensor or an int."""
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not x.is_cuda:
            raise TypeError("batch APIs take device (CUDA/HIP) tensors")
        return int(x.data_ptr())
    raise TypeError("expected a device tensor or an integer pointer")


def _host_ptr(x) -> int:
    """Host address of a numpy array, a CPU torch tensor (pinned or not) or an int."""
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return int(x.ctypes.data)
    if hasattr(x, "data_ptr"):
        if x.is_cuda:
            raise TypeError("host batch APIs take host (CPU) buffers")
        return int(x.data_ptr())
    raise TypeError("expected a host array/tensor or an integer pointer")


def _avail_bytes(x) -> Optional[int]:
    """Bytes addressable from the buffer's first byte to the end of its allocation:
    torch tensors use their storage, numpy arrays their outermost base array.
    None for raw integer pointers (the caller vouches for those)."""
    if isinstance(x, int):
        return None
    if isinstance(x, np.ndarray):
        base = x
        while isinstance(base.base, np.ndarray):
            base = base.base
        hi = base.ctypes.data + base.nbytes if base.flags.c_contiguous else None
        return None if hi is None else hi - x.ctypes.data
    if hasattr(x, "untyped_storage"):
        st = x.untyped_storage()
        return st.data_ptr() + st.nbytes() - x.data_ptr()
    return None


def _check_layout(buf, stripe_stride, slot_stride, max_slot, nstripes, nbytes, what):
    """Fail loudly (ArrayIndexOutOfBoundsException, as a Java ByteBuffer would)
    instead of letting a kernel address past the end of `buf`."""
    if nstripes <= 0 or nbytes <= 0:
        return
    if stripe_stride < 0 or slot_stride < 0:
        raise EcxError(-1, f"{what}: negative stride")
    avail = _avail_bytes(buf)
    need = (nstripes - 1) * stripe_stride + max(0, max_slot) * slot_stride + nbytes
    if avail is not None and need > avail:
        raise EcxError(-5, f"{what}: the batch layout addresses {need} bytes but the buffer holds {avail}")


def _check_extent(buf, nbytes, what):
    avail = _avail_bytes(buf)
    if nbytes > 0 and avail is not None and nbytes > avail:
        raise EcxError(-5, f"{what}: the batch addresses {nbytes} bytes but the buffer holds {avail}")


def pair_index(n: int, i: int, j: int) -> int:
    """The place of the pair {i, j}, i < j, among the C(n,2) pairs of n shards in lexicographic
    order: locateCorrupt2Batch's suspect n + pair_index(n, i, j) and doubleLossPatternSet()'s pattern."""
    if not 0 <= i < j < n:
        raise ValueError("pair_index needs 0 <= i < j < n")
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def pair_of(n: int, p: int):
    """The pair (i, j) with pair_index(n, i, j) == p."""
    if not 0 <= p < n * (n - 1) // 2:
        raise ValueError("pair_of needs 0 <= p < C(n,2)")
    i = 0
    while p >= n - 1 - i:
        p -= n - 1 - i
        i += 1
    return i, i + 1 + p


def blocked_pack(shards, block_bytes: int, out=None):
    """The blocked layout (include/ecx.h ecx_rs_blocked_layout) of a [stripes][n][L] uint8
    tensor, as a flat tensor of stripes * n * L bytes: body [stripe][block][shard][block_bytes],
    then tails [stripe][shard][L % block_bytes] (torch copies on the tensor's device)."""
    S, n, L = shards.shape
    full, tail = divmod(L, block_bytes)
    if out is None:
        out = shards.new_empty(S * n * L)
    body = full * n * block_bytes
    if full:
        out[:S * body].view(S, full, n, block_bytes).copy_(
            shards[:, :, :full * block_bytes].reshape(S, n, full, block_bytes).permute(0, 2, 1, 3))
    if tail:
        out[S * body:].view(S, n, tail).copy_(shards[:, :, full * block_bytes:])
    return out


def blocked_unpack(flat, stripes: int, n: int, byte_count: int, block_bytes: int, slots=None, first: int = 0,
                   count: int = None):
    """The natural [count][len(slots)][byte_count] shards (default: every stripe, every slot) of
    stripes first..first+count-1 of a blocked-layout buffer of `stripes` stripes (a copy)."""
    import torch
    count = stripes - first if count is None else count
    slots = list(range(n)) if slots is None else list(slots)
    full, tail = divmod(byte_count, block_bytes)
    body = full * n * block_bytes
    parts = []
    if full:
        b = flat[:stripes * body].view(stripes, full, n, block_bytes)[first:first + count][:, :, slots, :]
        parts.append(b.permute(0, 2, 1, 3).reshape(count, len(slots), full * block_bytes))
    if tail:
        t = flat[stripes * body:stripes * n * byte_count].view(stripes, n, tail)[first:first + count]
        parts.append(t[:, slots, :])
    return torch.cat(parts, dim=2) if len(parts) > 1 else parts[0].clone()


class HostBuffer:
    """Page-locked host memory from ecx_host_alloc, viewed as a numpy uint8 array."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        check(lib().ecx_host_alloc(nbytes, ctypes.byref(p)))
        self._p = p
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * max(1, nbytes)).from_address(p.value))[:nbytes]

    def __del__(self):
        if getattr(self, "_p", None) and lib is not None:
            lib().ecx_host_free(self._p)
            self._p = None


def host_register(arr) -> None:
    """Page-lock an existing host buffer (hipHostRegister) for PCIe-rate host batches."""
    check(lib().ecx_host_register(_host_ptr(arr), int(arr.nbytes)))


def host_unregister(arr) -> None:
    check(lib().ecx_host_unregister(_host_ptr(arr)))


def tune(key: str, value: int) -> None:
    """Launch-shape knobs (include/ecx_tune.h); results are bit-identical for every setting."""
    f = lib().ecx_tune
    f.argtypes, f.restype = [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    check(f(key.encode(), int(value)))


def tune_value(key: str) -> int:
    """The current value of a deployment knob (ecx_tune_value, include/ecx_tune.h)."""
    f = lib().ecx_tune_value
    f.argtypes, f.restype = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)], ctypes.c_int
    v = ctypes.c_int()
    check(f(key.encode(), ctypes.byref(v)))
    return v.value


def is_diag() -> bool:
    """True for the diagnostic library (make DIAG=1, libecx_diag.so): it also holds the
    measured-and-rejected kernels, whose ecx_tune keys the product library refuses."""
    f = lib().ecx_build_diag
    f.argtypes, f.restype = [], ctypes.c_int
    return f() == 1


def last_kernel() -> str:
    """The kernel instance of this thread's last full-chunk launch, as rocprofv3 names it
    (ecx_last_kernel, include/ecx_tune.h); "" before the first launch."""
    f = lib().ecx_last_kernel
    f.argtypes, f.restype = [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    buf = ctypes.create_string_buffer(256)
    return buf.value.decode() if check(f(buf, len(buf))) > 0 else ""


def last_launch_shape() -> str:
    """That launch's full shape: kernel instance plus the unit order its name does not encode
    ("... stagger=G xcd_group=X xcd_run=R"; ecx_last_launch_shape)."""
    f = lib().ecx_last_launch_shape
    f.argtypes, f.restype = [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    buf = ctypes.create_string_buffer(512)
    return buf.value.decode() if check(f(buf, len(buf))) > 0 else ""


def probe_bandwidth(kind: int, src, dst, nbytes: int, nontemporal: bool = True, stream=None) -> None:
    """Pure-bandwidth probe kernels (include/ecx_tune.h): kind 0 = read-only stream of
    `src`, kind 1 = copy src -> dst; nbytes a multiple of 16 KiB.  Diagnostics only."""
    f = lib().ecx_probe_bandwidth
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    f.restype = ctypes.c_int
    check(f(kind, _dev_ptr(src), _dev_ptr(dst), nbytes, 1 if nontemporal else 0, _stream(stream)))


def _stream(stream) -> Optional[int]:
    if stream is None:
        try:
            import torch
            return int(torch.cuda.current_stream().cuda_stream)
        except Exception:  # pragma: no cover - no torch / no device
            return None
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)


def device_count() -> int:
    n = ctypes.c_int(0)
    check(lib().ecx_device_count(ctypes.byref(n)))
    return n.value


def set_device(device: int) -> None:
    check(lib().ecx_set_device(device))


def fill_random(dst, nbytes: int, seed: int, stream=None) -> None:
    """Deterministic counter-based synthetic bytes on the device (splitmix64)."""
    check(lib().ecx_fill_random(_dev_ptr(dst), nbytes, seed & 0xFFFFFFFFFFFFFFFF, _stream(stream)))


def count_mismatch(a, a_stride, b, b_stride, nrows, row_bytes, d_count, stream=None) -> None:
    """Accumulate into the device uint64 ``d_count`` the bytes that differ."""
    check(lib().ecx_count_mismatch(_dev_ptr(a), a_stride, None if b is None else _dev_ptr(b), b_stride, nrows,
                                   row_bytes, _dev_ptr(d_count), _stream(stream)))


# ---------------------------------------------------------------- Galois.java
class Galois:
    """GF(2^8) with generating polynomial 29 (Galois.java:43)."""
    FIELD_SIZE = 256
    GENERATING_POLYNOMIAL = 29

    @staticmethod
    def multiply(a: int, b: int) -> int:
        return lib().ecx_gf_multiply(a & 0xFF, b & 0xFF)

    @staticmethod
    def divide(a: int, b: int) -> int:
        return check(lib().ecx_gf_divide(a & 0xFF, b & 0xFF))

    @staticmethod
    def exp(a: int, n: int) -> int:
        return check(lib().ecx_gf_exp(a & 0xFF, n))

    @staticmethod
    def add(a: int, b: int) -> int:
        return (a ^ b) & 0xFF

    subtract = add

    @staticmethod
    def tables():
        log = np.zeros(256, np.int16)
        exp = np.zeros(510, np.uint8)
        mul = np.zeros((256, 256), np.uint8)
        check(lib().ecx_gf_tables(log.ctypes.data, exp.ctypes.data, mul.ctypes.data))
        return log, exp, mul


# ---------------------------------------------------------------- Matrix.java
class Matrix:
    @staticmethod
    def times(a, b) -> np.ndarray:
        a, b = _bytes(a), _bytes(b)
        out = np.zeros((a.shape[0], b.shape[1]), np.uint8)
        check(lib().ecx_matrix_times(a.ctypes.data, a.shape[0], a.shape[1], b.ctypes.data, b.shape[0], b.shape[1],
                                     out.ctypes.data))
        return out

    @staticmethod
    def invert(m) -> np.ndarray:
        m = _bytes(m)
        out = np.zeros_like(m)
        check(lib().ecx_matrix_invert(m.ctypes.data, m.shape[0], out.ctypes.data))
        return out


# ---------------------------------------------------------------- CodingLoop.java
class CodingLoop:
    """The reference's operator/plugin interface (CodingLoop.java:79-117),
    implemented by one fused HIP kernel launch per call."""

    def codeSomeShards(self, matrixRows, inputs, inputCount, outputs, outputCount, offset, byteCount):
        m = _bytes([list(matrixRows[o])[:inputCount] for o in range(outputCount)]).reshape(outputCount, inputCount)
        check(lib().ecx_code_some_shards(m.ctypes.data, _ptr_array(inputs[:inputCount]), inputCount,
                                         _ptr_array(outputs[:outputCount]), outputCount, offset, byteCount))

    def checkSomeShards(self, matrixRows, inputs, inputCount, toCheck, checkCount, offset, byteCount,
                        tempBuffer=None) -> bool:
        m = _bytes([list(matrixRows[o])[:inputCount] for o in range(checkCount)]).reshape(checkCount, inputCount)
        return bool(check(lib().ecx_check_some_shards(m.ctypes.data, _ptr_array(inputs[:inputCount]), inputCount,
                                                      _ptr_array(toCheck[:checkCount]), checkCount, offset,
                                                      byteCount, None)))


InputOutputByteTableCodingLoop = CodingLoop  # the default loop of ReedSolomon.create (ReedSolomon.java:35)


class InputOutputByteTableCodingLoopSingle:
    """InputOutputByteTableCodingLoopSingle.java:4-20."""

    def codeSomeShards(self, matrixRows, input, index, output, outputIndex, offset, byteCount, isFirstTime):
        rows = [list(r) for r in matrixRows]
        width = max(len(r) for r in rows)
        m = _bytes([r + [0] * (width - len(r)) for r in rows])
        check(lib().ecx_code_single(m.ctypes.data, width, _u8(input).ctypes.data, index, _u8(output).ctypes.data,
                                    outputIndex, offset, byteCount, 1 if isFirstTime else 0))


# ---------------------------------------------------------------- compiled maps
class GfMap:
    """A compiled GF(256) linear map resident on the device (ecx_map)."""

    def __init__(self, handle, owner=None, owned=False):
        self._h = handle
        self._owner = owner  # keeps a codec alive while its maps are used
        self._owned = owned

    @classmethod
    def from_matrix(cls, matrix, in_slot=None, out_slot=None) -> "GfMap":
        m = _bytes(matrix)
        n_out, n_in = m.shape
        ins = None if in_slot is None else np.ascontiguousarray(in_slot, np.int32)
        outs = None if out_slot is None else np.ascontiguousarray(out_slot, np.int32)
        h = ctypes.c_void_p()
        check(lib().ecx_map_create(m.ctypes.data, n_out, n_in, None if ins is None else ins.ctypes.data,
                                   None if outs is None else outs.ctypes.data, ctypes.byref(h)))
        g = cls(h, owned=True)
        g._keep = (ins, outs)
        return g

    def __del__(self):
        if getattr(self, "_owned", False) and self._h and lib is not None:
            lib().ecx_map_destroy(self._h)
            self._h = None

    def info(self):
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().ecx_map_info(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"n_out": a.value, "n_in": b.value, "nnz": c.value}

    def accumulate_batch(self, inp, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride,
                         nstripes, byte_count, stream=None):
        """out ^= M * in (partial sums)."""
        self._check(inp, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride, nstripes,
                    byte_count)
        check(lib().ecx_map_accumulate_batch(self._h, _dev_ptr(inp), in_stripe_stride, in_slot_stride,
                                             _dev_ptr(out), out_stripe_stride, out_slot_stride, nstripes,
                                             byte_count, _stream(stream)))

    def matrix(self):
        """(dense matrix n_out x n_in, in_slot, out_slot) of the composed map."""
        inf = self.info()
        m = np.zeros((inf["n_out"], inf["n_in"]), np.uint8)
        ins = np.zeros(max(1, inf["n_in"]), np.int32)
        outs = np.zeros(max(1, inf["n_out"]), np.int32)
        check(lib().ecx_map_matrix(self._h, m.ctypes.data, ins.ctypes.data, outs.ctypes.data))
        return m, ins[:inf["n_in"]].copy(), outs[:inf["n_out"]].copy()

    def max_slots(self):
        """(largest input slot, largest output slot) of the map (cached)."""
        if getattr(self, "_max_slots", None) is None:
            _, ins, outs = self.matrix()
            self._max_slots = (int(ins.max()) if len(ins) else 0, int(outs.max()) if len(outs) else 0)
        return self._max_slots

    def selftest(self, seed: int = 1) -> None:
        """Host-only check that the compiled plan (tables, tiles, tile-group unions)
        reproduces the dense map (ecx_map_selftest, include/ecx_tune.h)."""
        f = lib().ecx_map_selftest
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_uint64], ctypes.c_int
        check(f(self._h, seed))

    def planes_compile_check(self, accumulate: bool = False) -> int:
        """Generate this map's bit-plane kernel (k_map_planes) and compile it with hiprtc
        for gfx950; returns the code-object size (ecx_map_planes_compile_check)."""
        f = lib().ecx_map_planes_compile_check
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
        return check(f(self._h, int(accumulate)))

    def planes_source(self, accumulate: bool = False) -> str:
        """The generated k_map_planes source (ecx_map_planes_source)."""
        f = lib().ecx_map_planes_source
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int], ctypes.c_int
        n = check(f(self._h, int(accumulate), None, 0))
        buf = ctypes.create_string_buffer(n + 1)
        check(f(self._h, int(accumulate), buf, n + 1))
        return buf.value.decode()

    def plan_stats(self) -> dict:
        """Shape of the compiled plan (ecx_map_plan_stats, include/ecx_tune.h)."""
        f = lib().ecx_map_plan_stats
        f.argtypes, f.restype = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 4, ctypes.c_int
        v = [ctypes.c_int() for _ in range(4)]
        check(f(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(["tiles", "entries", "groups", "union_total"], [x.value for x in v]))

    def layout_choice(self, slot_pitch: int, with_times: bool = False):
        """The launch shape "layout_select" kept for the latest selected batch layout of this
        map at an input slot pitch (ecx_map_layout_choice, include/ecx_tune.h): -1 none yet,
        0x100 the static rules' shape, else shape + 8 * stagger (shape 0 256-thread / 4 KiB
        workgroups, 1 skewed chunks, 2 one-wave / 1 KiB workgroups).  with_times: also the
        per-candidate median launch times (ms, -1 unsampled)."""
        f = lib().ecx_map_layout_choice
        f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
        f.restype = ctypes.c_int
        ms = (ctypes.c_float * 8)()
        c = check(f(self._h, int(slot_pitch), ms if with_times else None, 8 if with_times else 0))
        if c == 0x200:
            c = -1  # none chosen yet
        return (c, [round(float(x), 4) for x in ms]) if with_times else c

    def host_plan(self, in_stripe_stride, in_slot_stride, out_stripe_stride, out_slot_stride, nstripes, byte_count):
        """How apply_batch_host would move this batch (ecx_map_host_plan, host-only): a dict of the
        stripes per chunk, the chunk count, the buffer sets, and per chunk the H2D / D2H strided
        copies with the most rows per stripe one copy moves (> 1 where runs are folded or copied in
        3D) and how many of them are 3D."""
        f = lib().ecx_map_host_plan
        f.argtypes = [ctypes.c_void_p] + [ctypes.c_int64] * 6 + [ctypes.c_void_p]
        f.restype = ctypes.c_int
        out = np.zeros(10, np.int64)
        check(f(self._h, in_stripe_stride, in_slot_stride, out_stripe_stride, out_slot_stride, nstripes, byte_count,
                out.ctypes.data))
        keys = ("chunk", "chunks", "buffers", "h2d_copies", "h2d_rows", "d2h_copies", "d2h_rows", "h2d_3d", "d2h_3d",
                "slices")
        return {k: int(v) for k, v in zip(keys, out)}

    def launch_plan(self, in_addr, in_stripe_stride, in_slot_stride, out_addr, out_stripe_stride, out_slot_stride,
                    nstripes, byte_count, accumulate: bool = False, cand: int = 0) -> str:
        """What last_launch_shape() would report after apply_batch (accumulate_batch) of this layout
        under the current knobs (ecx_map_launch_plan, host-only: nothing is launched).  The buffers
        are given as integer addresses; cand is the "layout_select" candidate, 0 = the static
        rules.  "" for a call that launches no full-chunk kernel."""
        f = lib().ecx_map_launch_plan
        I64, U64 = ctypes.c_int64, ctypes.c_uint64
        f.argtypes = [ctypes.c_void_p, U64, I64, I64, U64, I64, I64, I64, I64, ctypes.c_int, ctypes.c_int,
                      ctypes.c_char_p, ctypes.c_int]
        f.restype = ctypes.c_int
        buf = ctypes.create_string_buffer(512)
        n = check(f(self._h, int(in_addr), in_stripe_stride, in_slot_stride, int(out_addr), out_stripe_stride,
                    out_slot_stride, nstripes, byte_count, int(bool(accumulate)), int(cand), buf, len(buf)))
        return buf.value.decode() if n > 0 else ""

    def layout_state(self, slot_pitch: int):
        """(state, dropped probes) of that layout's selection (ecx_map_layout_state): state -1
        none yet, 0 exploring, 1 chosen, 2 re-validating, 3 re-validated, 4 contended."""
        f = lib().ecx_map_layout_state
        f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        f.restype = ctypes.c_int
        st, dr = ctypes.c_int(), ctypes.c_int()
        check(f(self._h, int(slot_pitch), ctypes.byref(st), ctypes.byref(dr)))
        return st.value, dr.value

    def _check(self, inp, iss, isl, out, oss, osl, nstripes, nbytes):
        mi, mo = self.max_slots()
        _check_layout(inp, iss, isl, mi, nstripes, nbytes, "input")
        _check_layout(out, oss, osl, mo, nstripes, nbytes, "output")

    def apply_batch(self, inp, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride, nstripes,
                    byte_count, stream=None):
        self._check(inp, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride, nstripes,
                    byte_count)
        check(lib().ecx_map_apply_batch(self._h, _dev_ptr(inp), in_stripe_stride, in_slot_stride, _dev_ptr(out),
                                        out_stripe_stride, out_slot_stride, nstripes, byte_count, _stream(stream)))

    def apply_batch_host(self, inp, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride,
                         nstripes, byte_count):
        """apply_batch over host buffers: pipelined H2D -> kernel -> D2H, synchronous."""
        self._check(inp, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride, nstripes,
                    byte_count)
        check(lib().ecx_map_apply_batch_host(self._h, _host_ptr(inp), in_stripe_stride, in_slot_stride,
                                             _host_ptr(out), out_stripe_stride, out_slot_stride, nstripes,
                                             byte_count))

    def apply_batch_host_devices(self, inp, in_stripe_stride, in_slot_stride, out, out_stripe_stride,
                                 out_slot_stride, nstripes, byte_count, devices):
        """apply_batch_host split over several GPUs (ecx_map_apply_batch_host_devices): device j
        of ``devices`` takes the contiguous stripe range shard_stripes(nstripes, len(devices), j)
        on a worker thread of its own -- or, with fewer stripes than entries, a contiguous range of
        every slot's bytes (4 KiB units); synchronous."""
        self._check(inp, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride, nstripes,
                    byte_count)
        devs = list(devices)
        arr = np.ascontiguousarray(devs + [0], np.int32)  # never a null list: an empty one is ndev 0
        check(lib().ecx_map_apply_batch_host_devices(self._h, _host_ptr(inp), in_stripe_stride, in_slot_stride,
                                                     _host_ptr(out), out_stripe_stride, out_slot_stride, nstripes,
                                                     byte_count, arr.ctypes.data, len(devs)))


# ---------------------------------------------------------------- ReedSolomon.java
class ReedSolomon:
    """ReedSolomon.java: systematic RS over GF(2^8), Vandermonde-derived."""

    def __init__(self, dataShardCount: int, parityShardCount: int, codingLoop=None):
        h = ctypes.c_void_p()
        check(lib().ecx_rs_create(dataShardCount, parityShardCount, ctypes.byref(h)))
        self._h = h
        self.dataShardCount = dataShardCount
        self.parityShardCount = parityShardCount
        self.totalShardCount = dataShardCount + parityShardCount

    @classmethod
    def create(cls, dataShardCount: int, parityShardCount: int) -> "ReedSolomon":
        return cls(dataShardCount, parityShardCount)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().ecx_rs_destroy(self._h)
            self._h = None

    def getDataShardCount(self):
        return self.dataShardCount

    def getParityShardCount(self):
        return self.parityShardCount

    def getTotalShardCount(self):
        return self.totalShardCount

    @property
    def matrix(self) -> np.ndarray:
        out = np.zeros((self.totalShardCount, self.dataShardCount), np.uint8)
        check(lib().ecx_rs_matrix(self._h, out.ctypes.data))
        return out

    @property
    def parityRows(self) -> np.ndarray:
        return self.matrix[self.dataShardCount:]

    @staticmethod
    def _len(shards):
        return len(shards[0]) if len(shards) and shards[0] is not None else 0

    def encodeParity(self, shards, offset: int, byteCount: int) -> None:
        check(lib().ecx_rs_encode_parity(self._h, _ptr_array(shards), len(shards), self._len(shards), offset,
                                         byteCount))

    def encodeParitySingle(self, shard, output, inputIndex, outputIndex, offset, byteCount) -> None:
        check(lib().ecx_rs_encode_parity_single(self._h, _u8(shard).ctypes.data, _u8(output).ctypes.data,
                                                inputIndex, outputIndex, offset, byteCount))

    def isParityCorrect(self, shards, firstByte: int, byteCount: int, tempBuffer=None) -> bool:
        t = None if tempBuffer is None else _u8(tempBuffer).ctypes.data
        tl = 0 if tempBuffer is None else len(tempBuffer)
        return bool(check(lib().ecx_rs_is_parity_correct(self._h, _ptr_array(shards), len(shards),
                                                         self._len(shards), firstByte, byteCount, t, tl)))

    def decodeMissing(self, shards, shardPresent, offset: int, byteCount: int) -> None:
        pres = np.array([1 if p else 0 for p in shardPresent], np.uint8)
        check(lib().ecx_rs_decode_missing(self._h, _ptr_array(shards), pres.ctypes.data, len(shards),
                                          self._len(shards), offset, byteCount))

    def decodeMissingSingle(self, shard, shardIndex, index, shardPresent, outputs, offset, byteCount,
                            isFirst) -> None:
        pres = np.array([1 if p else 0 for p in shardPresent], np.uint8)
        check(lib().ecx_rs_decode_missing_single(self._h, _u8(shard).ctypes.data, shardIndex, index,
                                                 pres.ctypes.data, _ptr_array(outputs), len(outputs), offset,
                                                 byteCount, 1 if isFirst else 0))

    # batched, device-resident
    def encodeParityBatch(self, shards, stripe_stride, shard_stride, nstripes, offset, byteCount, stream=None):
        """encodeParity over nstripes device-resident stripes, in place (ecx_rs_encode_parity_batch)."""
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes, offset + byteCount,
                      "shards")
        check(lib().ecx_rs_encode_parity_batch(self._h, _dev_ptr(shards), stripe_stride, shard_stride, nstripes,
                                               offset, byteCount, _stream(stream)))

    # ---- the blocked layout contract (ecx_rs_blocked_layout, include/ecx.h)
    def blockedLayout(self, byteCount: int):
        """(block_bytes, full blocks, tail bytes) of the recommended blocked layout of this
        code's stripes for a shard size (ecx_rs_blocked_layout)."""
        out = np.zeros(3, np.int64)
        check(lib().ecx_rs_blocked_layout(self.dataShardCount, self.parityShardCount, byteCount, out.ctypes.data))
        return int(out[0]), int(out[1]), int(out[2])

    def recommendedPitch(self, byteCount: int) -> int:
        """The recommended shard pitch of the plain [stripe][shard][pitch] layout (ecx_rs_recommended_pitch)."""
        out = np.zeros(1, np.int64)
        check(lib().ecx_rs_recommended_pitch(self.dataShardCount, self.parityShardCount, byteCount,
                                             out.ctypes.data))
        return int(out[0])

    def encodeParityBlockedBatch(self, base, nstripes, byteCount, blockBytes=0, stream=None):
        """encodeParity over nstripes stripes in the blocked layout, in place
        (ecx_rs_encode_parity_blocked_batch; blockBytes 0 = the recommended block)."""
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        check(lib().ecx_rs_encode_parity_blocked_batch(self._h, _dev_ptr(base), nstripes, byteCount, blockBytes,
                                                       _stream(stream)))

    def decodeMissingBlockedBatch(self, base, shardPresent, nstripes, byteCount, blockBytes=0, stream=None):
        """decodeMissing over nstripes stripes in the blocked layout, in place
        (ecx_rs_decode_missing_blocked_batch)."""
        pres = np.array([1 if p else 0 for p in shardPresent], np.uint8)
        if len(pres) != self.getTotalShardCount():
            raise EcxError(-1, "wrong number of shardPresent flags")
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        check(lib().ecx_rs_decode_missing_blocked_batch(self._h, pres.ctypes.data, _dev_ptr(base), nstripes,
                                                        byteCount, blockBytes, _stream(stream)))

    def encodeParityBlockedBatchHost(self, base, nstripes, byteCount, blockBytes=0):
        """encodeParityBlockedBatch over HOST-memory stripes in the blocked layout, in place
        (ecx_rs_encode_parity_blocked_batch_host: the full blocks, then the tails, each a
        pipelined host batch)."""
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        check(lib().ecx_rs_encode_parity_blocked_batch_host(self._h, _host_ptr(base), nstripes, byteCount,
                                                            blockBytes))

    def decodeMissingBlockedBatchHost(self, base, shardPresent, nstripes, byteCount, blockBytes=0):
        """decodeMissingBlockedBatch over HOST-memory stripes, in place
        (ecx_rs_decode_missing_blocked_batch_host)."""
        pres = np.array([1 if p else 0 for p in shardPresent], np.uint8)
        if len(pres) != self.getTotalShardCount():
            raise EcxError(-1, "wrong number of shardPresent flags")
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        check(lib().ecx_rs_decode_missing_blocked_batch_host(self._h, pres.ctypes.data, _host_ptr(base), nstripes,
                                                             byteCount, blockBytes))

    def encodeParityBlockedBatchHostDevices(self, base, nstripes, byteCount, devices, blockBytes=0):
        """encodeParityBlockedBatchHost split over several GPUs of this process
        (ecx_rs_encode_parity_blocked_batch_host_devices): contiguous stripe ranges, one worker
        thread and pipe per device entry."""
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        devs = list(devices)
        arr = np.ascontiguousarray(devs + [0], np.int32)  # never a null list: an empty one is ndev 0
        check(lib().ecx_rs_encode_parity_blocked_batch_host_devices(self._h, _host_ptr(base), nstripes, byteCount,
                                                                    blockBytes, arr.ctypes.data, len(devs)))

    def decodeMissingBlockedBatchHostDevices(self, base, shardPresent, nstripes, byteCount, devices, blockBytes=0):
        """decodeMissingBlockedBatchHost split over several GPUs of this process
        (ecx_rs_decode_missing_blocked_batch_host_devices)."""
        pres = np.array([1 if p else 0 for p in shardPresent], np.uint8)
        if len(pres) != self.getTotalShardCount():
            raise EcxError(-1, "wrong number of shardPresent flags")
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        devs = list(devices)
        arr = np.ascontiguousarray(devs + [0], np.int32)
        check(lib().ecx_rs_decode_missing_blocked_batch_host_devices(self._h, pres.ctypes.data, _host_ptr(base),
                                                                     nstripes, byteCount, blockBytes,
                                                                     arr.ctypes.data, len(devs)))

    def isParityCorrectBatch(self, shards, stripe_stride, shard_stride, nstripes, firstByte, byteCount, verdict,
                             stream=None) -> None:
        """isParityCorrect over nstripes device-resident stripes, read-only
        (ecx_rs_is_parity_correct_batch): the device uint8 array ``verdict`` (nstripes bytes)
        receives 1 for each stripe whose parity is correct over [firstByte, firstByte +
        byteCount), else 0.  Enqueued on ``stream``; read verdict after synchronising."""
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes,
                      firstByte + byteCount, "shards")
        _check_layout(verdict, 1, 0, 0, nstripes, 1, "verdict")
        check(lib().ecx_rs_is_parity_correct_batch(self._h, _dev_ptr(shards), stripe_stride, shard_stride, nstripes,
                                                   firstByte, byteCount, _dev_ptr(verdict), _stream(stream)))

    def isParityCorrectBatchHost(self, shards, stripe_stride, shard_stride, nstripes, firstByte, byteCount,
                                 verdict) -> None:
        """isParityCorrectBatch over HOST-memory stripes (ecx_rs_is_parity_correct_batch_host):
        chunks of stripes are pipelined H2D through the read-only check kernel and only the
        verdict bytes come back into the host uint8 array ``verdict`` (nstripes bytes)."""
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes,
                      firstByte + byteCount, "shards")
        _check_layout(verdict, 1, 0, 0, nstripes, 1, "verdict")
        check(lib().ecx_rs_is_parity_correct_batch_host(self._h, _host_ptr(shards), stripe_stride, shard_stride,
                                                        nstripes, firstByte, byteCount, _host_ptr(verdict)))

    def isParityCorrectBatchHostDevices(self, shards, stripe_stride, shard_stride, nstripes, firstByte, byteCount,
                                        verdict, devices) -> None:
        """isParityCorrectBatchHost split over several GPUs of this process
        (ecx_rs_is_parity_correct_batch_host_devices): contiguous stripe ranges, one worker
        thread and pipe per device entry."""
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes,
                      firstByte + byteCount, "shards")
        _check_layout(verdict, 1, 0, 0, nstripes, 1, "verdict")
        devs = list(devices)
        arr = np.ascontiguousarray(devs + [0], np.int32)  # never a null list: an empty one is ndev 0
        check(lib().ecx_rs_is_parity_correct_batch_host_devices(self._h, _host_ptr(shards), stripe_stride,
                                                                shard_stride, nstripes, firstByte, byteCount,
                                                                _host_ptr(verdict), arr.ctypes.data, len(devs)))

    def isParityCorrectBlockedBatch(self, base, nstripes, byteCount, verdict, blockBytes=0, stream=None) -> None:
        """isParityCorrect over nstripes device-resident stripes in the blocked layout, read-only
        (ecx_rs_is_parity_correct_blocked_batch; blockBytes 0 = the recommended block): the device
        uint8 array ``verdict`` (nstripes bytes) receives 1 for each stripe whose natural shards
        pass isParityCorrect over [0, byteCount), else 0.  Enqueued on ``stream``."""
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        _check_layout(verdict, 1, 0, 0, nstripes, 1, "verdict")
        check(lib().ecx_rs_is_parity_correct_blocked_batch(self._h, _dev_ptr(base), nstripes, byteCount, blockBytes,
                                                           _dev_ptr(verdict), _stream(stream)))

    def isParityCorrectBlockedBatchHost(self, base, nstripes, byteCount, verdict, blockBytes=0) -> None:
        """isParityCorrectBlockedBatch over HOST-memory stripes in the blocked layout
        (ecx_rs_is_parity_correct_blocked_batch_host): the full blocks, then the tails, each a
        pipelined host check; only verdict bytes come back, into the host uint8 array ``verdict``."""
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        _check_layout(verdict, 1, 0, 0, nstripes, 1, "verdict")
        check(lib().ecx_rs_is_parity_correct_blocked_batch_host(self._h, _host_ptr(base), nstripes, byteCount,
                                                                blockBytes, _host_ptr(verdict)))

    def isParityCorrectBlockedBatchHostDevices(self, base, nstripes, byteCount, verdict, devices,
                                               blockBytes=0) -> None:
        """isParityCorrectBlockedBatchHost split over several GPUs of this process
        (ecx_rs_is_parity_correct_blocked_batch_host_devices): each pass over contiguous ranges,
        one worker thread and pipe per device entry."""
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        _check_layout(verdict, 1, 0, 0, nstripes, 1, "verdict")
        devs = list(devices)
        arr = np.ascontiguousarray(devs + [0], np.int32)  # never a null list: an empty one is ndev 0
        check(lib().ecx_rs_is_parity_correct_blocked_batch_host_devices(self._h, _host_ptr(base), nstripes,
                                                                        byteCount, blockBytes, _host_ptr(verdict),
                                                                        arr.ctypes.data, len(devs)))

    def _check_locate_outputs(self, nstripes, suspect, culprit, healId):
        n = self.getTotalShardCount()
        _check_layout(suspect, n, 0, 0, nstripes, n, "suspect")
        _check_layout(culprit, 4, 0, 0, nstripes, 4, "culprit")
        if healId is not None:
            _check_layout(healId, 1, 0, 0, nstripes, 1, "healId")

    def locateCorruptBatch(self, shards, stripe_stride, shard_stride, nstripes, firstByte, byteCount, suspect,
                           culprit, healId=None, stream=None) -> None:
        """Which shard of each stripe that fails isParityCorrect is corrupt, read-only
        (ecx_rs_locate_corrupt_batch; layout of isParityCorrectBatch, bytes [firstByte, firstByte +
        byteCount)).  ``suspect`` (device uint8 [nstripes][n]) receives 1 where replacing that shard
        alone can make the stripe pass; ``culprit`` (device int32, nstripes) -1 for a clean stripe,
        j for exactly one suspect, -2 when no single shard explains the stripe; ``healId`` (device
        uint8, nstripes, or None) j or 255 -- the ids that decodeMissingBatchMixed takes with
        singleLossPatternSet() to heal the batch on the same stream.  Codes with 2 <= m <= 8."""
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes,
                      firstByte + byteCount, "shards")
        self._check_locate_outputs(nstripes, suspect, culprit, healId)
        check(lib().ecx_rs_locate_corrupt_batch(self._h, _dev_ptr(shards), stripe_stride, shard_stride, nstripes,
                                                firstByte, byteCount, _dev_ptr(suspect), _dev_ptr(culprit),
                                                None if healId is None else _dev_ptr(healId), _stream(stream)))

    def locateCorruptBlockedBatch(self, base, nstripes, byteCount, suspect, culprit, healId=None, blockBytes=0,
                                  stream=None) -> None:
        """locateCorruptBatch over nstripes device-resident stripes in the blocked layout
        (ecx_rs_locate_corrupt_blocked_batch; blockBytes 0 = the recommended block), over bytes
        [0, byteCount) of the natural shards; ``healId`` feeds decodeMissingBlockedBatchMixed."""
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        self._check_locate_outputs(nstripes, suspect, culprit, healId)
        check(lib().ecx_rs_locate_corrupt_blocked_batch(self._h, _dev_ptr(base), nstripes, byteCount, blockBytes,
                                                        _dev_ptr(suspect), _dev_ptr(culprit),
                                                        None if healId is None else _dev_ptr(healId),
                                                        _stream(stream)))

    def singleLossPatternSet(self) -> "PatternSet":
        """The n patterns "shard j missing", in shard order (1 - eye(n)): pattern j rebuilds shard
        j, so locateCorruptBatch's healId names the pattern that heals each stripe, and 255 -- no
        pattern of this set -- leaves a stripe untouched."""
        n = self.getTotalShardCount()
        return self.patternSet(1 - np.eye(n, dtype=np.uint8))

    def _check_locate2_outputs(self, nstripes, suspect, culprit, healId):
        n = self.getTotalShardCount()
        width = n + n * (n - 1) // 2
        _check_layout(suspect, width, 0, 0, nstripes, width, "suspect")
        _check_layout(culprit, 8, 0, 0, nstripes, 8, "culprit")
        if healId is not None:
            _check_layout(healId, 1, 0, 0, nstripes, 1, "healId")

    def locateCorrupt2Batch(self, shards, stripe_stride, shard_stride, nstripes, firstByte, byteCount, suspect,
                            culprit, healId=None, stream=None) -> None:
        """Which one or two shards of each stripe that fails isParityCorrect are corrupt, read-only
        (ecx_rs_locate_corrupt2_batch; arguments of locateCorruptBatch).  ``suspect`` (device uint8
        [nstripes][n + C(n,2)]) receives the n single suspects, then 1 at n + pair_index(n, i, j)
        where replacing shards i and j together can make the stripe pass; ``culprit`` (device int32,
        2 * nstripes) (-1, -1) for a clean stripe, (j, -1) for one corrupt shard, (i, j) for two,
        (-2, -2) otherwise; ``healId`` (device uint8, nstripes, or None) j, n + pair_index(n, i, j)
        or 255 -- the ids that decodeMissingBatchMixed takes with doubleLossPatternSet().  Codes
        with 4 <= m <= 8 and n <= 64; heal ids for n <= 22."""
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes,
                      firstByte + byteCount, "shards")
        self._check_locate2_outputs(nstripes, suspect, culprit, healId)
        check(lib().ecx_rs_locate_corrupt2_batch(self._h, _dev_ptr(shards), stripe_stride, shard_stride, nstripes,
                                                 firstByte, byteCount, _dev_ptr(suspect), _dev_ptr(culprit),
                                                 None if healId is None else _dev_ptr(healId), _stream(stream)))

    def locateCorrupt2BlockedBatch(self, base, nstripes, byteCount, suspect, culprit, healId=None, blockBytes=0,
                                   stream=None) -> None:
        """locateCorrupt2Batch over nstripes device-resident stripes in the blocked layout
        (ecx_rs_locate_corrupt2_blocked_batch; arguments of locateCorruptBlockedBatch); ``healId``
        feeds decodeMissingBlockedBatchMixed with doubleLossPatternSet()."""
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        self._check_locate2_outputs(nstripes, suspect, culprit, healId)
        check(lib().ecx_rs_locate_corrupt2_blocked_batch(self._h, _dev_ptr(base), nstripes, byteCount, blockBytes,
                                                         _dev_ptr(suspect), _dev_ptr(culprit),
                                                         None if healId is None else _dev_ptr(healId),
                                                         _stream(stream)))

    def doubleLossPatternSet(self) -> "PatternSet":
        """The n single-loss patterns in shard order (ids 0..n-1 mean what they mean in
        singleLossPatternSet()), then the C(n,2) patterns "shards i and j missing" in pair order:
        pattern n + pair_index(n, i, j) rebuilds both, so locateCorrupt2Batch's healId names the
        pattern that heals each stripe.  n + C(n,2) <= 256 patterns: n <= 22."""
        n = self.getTotalShardCount()
        rows = [1 - np.eye(n, dtype=np.uint8)]
        for p in range(n * (n - 1) // 2):
            row = np.ones((1, n), np.uint8)
            row[0, list(pair_of(n, p))] = 0
            rows.append(row)
        return self.patternSet(np.concatenate(rows))

    def decodeMissingBatch(self, shards, shardPresent, stripe_stride, shard_stride, nstripes, offset, byteCount,
                           stream=None):
        """decodeMissing over nstripes device-resident stripes, in place (ecx_rs_decode_missing_batch)."""
        pres = np.array([1 if p else 0 for p in shardPresent], np.uint8)
        if len(pres) != self.getTotalShardCount():
            raise EcxError(-1, "wrong number of shardPresent flags")
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes, offset + byteCount,
                      "shards")
        check(lib().ecx_rs_decode_missing_batch(self._h, pres.ctypes.data, _dev_ptr(shards), stripe_stride,
                                                shard_stride, nstripes, offset, byteCount, _stream(stream)))

    def patternSet(self, patterns) -> "PatternSet":
        """The erasure patterns ``patterns`` ([npatterns][n] shardPresent flags, 1..256 rows) of
        this code compiled into one device plan (ecx_rs_pattern_set_create), for
        decodeMissingBatchMixed.  Close it once the work enqueued with it has finished."""
        return PatternSet(self, patterns)

    def decodeMissingBatchMixed(self, shards, patternSet, ids, stripe_stride, shard_stride, nstripes, offset,
                                byteCount, stream=None):
        """decodeMissing over nstripes device-resident stripes that miss different shards, in
        place and in one launch (ecx_rs_decode_missing_batch_mixed): stripe s is decoded with
        pattern ``ids[s]`` of ``patternSet``; ``ids`` is a device uint8 array of nstripes.  An id
        without a pattern, or a pattern with nothing missing, leaves its stripe untouched."""
        if patternSet._h is None:
            raise EcxError(-6, "the pattern set is closed")
        if patternSet.totalShardCount != self.getTotalShardCount():
            raise EcxError(-1, "the pattern set belongs to another code")
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes, offset + byteCount,
                      "shards")
        _check_layout(ids, 1, 0, 0, nstripes, 1, "ids")
        check(lib().ecx_rs_decode_missing_batch_mixed(patternSet._h, _dev_ptr(ids), _dev_ptr(shards), stripe_stride,
                                                      shard_stride, nstripes, offset, byteCount, _stream(stream)))

    def _check_pattern_set(self, patternSet):
        if patternSet._h is None:
            raise EcxError(-6, "the pattern set is closed")
        if patternSet.totalShardCount != self.getTotalShardCount():
            raise EcxError(-1, "the pattern set belongs to another code")

    def decodeMissingBlockedBatchMixed(self, base, patternSet, ids, nstripes, byteCount, blockBytes=0, stream=None):
        """decodeMissingBatchMixed over nstripes device-resident stripes in the blocked layout, in
        place (ecx_rs_decode_missing_blocked_batch_mixed; blockBytes 0 = the recommended block):
        stripe s is decoded with pattern ``ids[s]`` of ``patternSet``; ``ids`` is a device uint8
        array of nstripes.  An id without a pattern, or a pattern with nothing missing, leaves its
        stripe untouched, body and tail."""
        self._check_pattern_set(patternSet)
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        _check_layout(ids, 1, 0, 0, nstripes, 1, "ids")
        check(lib().ecx_rs_decode_missing_blocked_batch_mixed(patternSet._h, _dev_ptr(ids), _dev_ptr(base), nstripes,
                                                              byteCount, blockBytes, _stream(stream)))

    def decodeMissingBatchMixedHost(self, shards, patternSet, ids, stripe_stride, shard_stride, nstripes, offset,
                                    byteCount):
        """decodeMissingBatchMixed over HOST-memory stripes, in place and synchronous
        (ecx_rs_decode_missing_mixed_batch_host): ``shards`` and ``ids`` (uint8, nstripes) are
        host buffers, pageable or pinned."""
        self._check_pattern_set(patternSet)
        _check_layout(shards, stripe_stride, shard_stride, self.getTotalShardCount() - 1, nstripes, offset + byteCount,
                      "shards")
        _check_layout(ids, 1, 0, 0, nstripes, 1, "ids")
        check(lib().ecx_rs_decode_missing_mixed_batch_host(patternSet._h, _host_ptr(ids), _host_ptr(shards),
                                                           stripe_stride, shard_stride, nstripes, offset, byteCount))

    def decodeMissingBlockedBatchMixedHost(self, base, patternSet, ids, nstripes, byteCount, blockBytes=0):
        """decodeMissingBlockedBatchMixed over HOST-memory stripes in the blocked layout, in place
        and synchronous (ecx_rs_decode_missing_blocked_mixed_batch_host)."""
        self._check_pattern_set(patternSet)
        _check_extent(base, nstripes * self.getTotalShardCount() * byteCount, "base")
        _check_layout(ids, 1, 0, 0, nstripes, 1, "ids")
        check(lib().ecx_rs_decode_missing_blocked_mixed_batch_host(patternSet._h, _host_ptr(ids), _host_ptr(base),
                                                                   nstripes, byteCount, blockBytes))

    def decodePartialBatch(self, shardPresent, shardIndex, inp, in_stripe_stride, acc, acc_stripe_stride,
                           acc_row_stride, nstripes, byteCount, isFirst, stream=None):
        """Batched decodeMissingSingle for every missing shard (data and parity)."""
        pres = np.array([1 if p else 0 for p in shardPresent], np.uint8)
        _check_layout(inp, in_stripe_stride, 0, 0, nstripes, byteCount, "input")
        _check_layout(acc, acc_stripe_stride, acc_row_stride, int((pres == 0).sum()) - 1, nstripes, byteCount, "acc")
        check(lib().ecx_rs_decode_partial_batch(self._h, pres.ctypes.data, shardIndex, _dev_ptr(inp),
                                                in_stripe_stride, _dev_ptr(acc), acc_stripe_stride, acc_row_stride,
                                                nstripes, byteCount, 1 if isFirst else 0, _stream(stream)))

    def decodePartialBatchMixed(self, patternSet, ids, shardOfStripe, inp, in_stripe_stride, in_shard_stride, acc,
                                acc_stripe_stride, acc_row_stride, nstripes, byteCount, isFirst, stream=None):
        """decodePartialBatch with a pattern and a helper shard index per stripe, in one launch
        (ecx_rs_decode_partial_batch_mixed): stripe s adds shard ``shardOfStripe[s]``'s contribution
        to every shard pattern ``ids[s]`` of ``patternSet`` misses; both are device uint8 arrays of
        nstripes.  The stripe's input is ``inp + s * in_stripe_stride + shardOfStripe[s] *
        in_shard_stride`` (in_shard_stride 0: this helper's own shards back to back).  An id without
        a pattern, a pattern with nothing missing, or a shard byte that is no shard leaves its
        stripe untouched; so do the rows past a pattern's missing count."""
        self._check_pattern_set(patternSet)
        n = self.getTotalShardCount()
        _check_layout(inp, in_stripe_stride, in_shard_stride, n - 1 if in_shard_stride else 0, nstripes, byteCount,
                      "input")
        _check_layout(acc, acc_stripe_stride, acc_row_stride, patternSet.info()[2] - 1, nstripes, byteCount, "acc")
        _check_layout(ids, 1, 0, 0, nstripes, 1, "ids")
        _check_layout(shardOfStripe, 1, 0, 0, nstripes, 1, "shardOfStripe")
        check(lib().ecx_rs_decode_partial_batch_mixed(patternSet._h, _dev_ptr(ids), _dev_ptr(shardOfStripe),
                                                      _dev_ptr(inp), in_stripe_stride, in_shard_stride, _dev_ptr(acc),
                                                      acc_stripe_stride, acc_row_stride, nstripes, byteCount,
                                                      1 if isFirst else 0, _stream(stream)))

    def encodePartialBatch(self, inputIndex, inp, in_stripe_stride, acc, acc_stripe_stride, acc_row_stride,
                           nstripes, byteCount, isFirst, stream=None):
        """Batched encodeParitySingle into every parity row."""
        _check_layout(inp, in_stripe_stride, 0, 0, nstripes, byteCount, "input")
        _check_layout(acc, acc_stripe_stride, acc_row_stride, self.parityShardCount - 1, nstripes, byteCount, "acc")
        check(lib().ecx_rs_encode_partial_batch(self._h, inputIndex, _dev_ptr(inp), in_stripe_stride,
                                                _dev_ptr(acc), acc_stripe_stride, acc_row_stride, nstripes,
                                                byteCount, 1 if isFirst else 0, _stream(stream)))

    def encode_map(self) -> GfMap:
        h = ctypes.c_void_p()
        check(lib().ecx_rs_encode_map(self._h, ctypes.byref(h)))
        return GfMap(h, owner=self)

    def decode_map(self, shardPresent) -> GfMap:
        pres = np.array([1 if p else 0 for p in shardPresent], np.uint8)
        h = ctypes.c_void_p()
        check(lib().ecx_rs_decode_map(self._h, pres.ctypes.data, ctypes.byref(h)))
        return GfMap(h, owner=self)


class PatternSet:
    """ecx_rs_pattern_set: erasure patterns of one ReedSolomon code as one device plan
    (ReedSolomon.patternSet).  It keeps its code alive; close() (idempotent) frees it."""

    def __init__(self, rs: ReedSolomon, patterns):
        pats = np.ascontiguousarray(np.asarray(patterns) != 0, dtype=np.uint8)
        if pats.ndim != 2 or pats.shape[1] != rs.getTotalShardCount():
            raise EcxError(-1, "patterns must be [npatterns][%d] shardPresent flags" % rs.getTotalShardCount())
        h = ctypes.c_void_p()
        self._h = None
        check(lib().ecx_rs_pattern_set_create(rs._h, pats.ctypes.data, pats.shape[0], ctypes.byref(h)))
        self._h = h
        self._rs = rs
        self.totalShardCount = rs.getTotalShardCount()

    def info(self):
        """(patterns, shards per stripe, most shards any pattern misses)."""
        if self._h is None:
            raise EcxError(-6, "the pattern set is closed")
        v = [ctypes.c_int() for _ in range(3)]
        check(lib().ecx_rs_pattern_set_info(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().ecx_rs_pattern_set_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def index_patterns(present, cap: int = 256):
    """(patterns, ids) of per-stripe shardPresent flags ``present`` ([nstripes][n]): the distinct
    rows in order of first appearance (at most ``cap``), and for each stripe the index of its
    row among them -- the inputs of ReedSolomon.patternSet and, once on the device, of
    decodeMissingBatchMixed (ecx_rs_index_patterns)."""
    pres = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8)
    if pres.ndim != 2 or pres.shape[1] < 1:
        raise EcxError(-1, "present must be [nstripes][n] flags")
    nstripes, n = pres.shape
    patterns = np.zeros((max(1, min(cap, 256)), n), np.uint8)
    ids = np.zeros(max(1, nstripes), np.uint8)
    count = ctypes.c_int()
    check(lib().ecx_rs_index_patterns(n, pres.ctypes.data if nstripes else patterns.ctypes.data, nstripes,
                                      patterns.ctypes.data, cap, ctypes.byref(count), ids.ctypes.data))
    return patterns[:count.value].copy(), ids[:nstripes].copy()


# ---------------------------------------------------------------- Clay
class ClayCodeUtil:
    """ClayCodeErasureDecodingStep.ClayCodeUtil (:676-944) index arithmetic."""

    def __init__(self, erasedIndexes, numDataUnits, numParityUnits):
        self.q = numParityUnits
        self.t = (numParityUnits + numDataUnits) // numParityUnits
        self.erasedIndexes = list(erasedIndexes)
        self.subPacketSize = self.q ** self.t

    def getSubPacketSize(self):
        return self.subPacketSize

    def getZVector(self, z):
        v = [0] * self.t
        for i in range(self.t - 1, -1, -1):
            v[i] = z % self.q
            z //= self.q
        return v

    def getZ(self, v):
        z = 0
        for x in v:
            z = z * self.q + x
        return z

    def getNodeIndex(self, x, y):
        return x + self.q * y

    def getNodeCoordinates(self, i):
        return [i % self.q, i // self.q]

    def getCouplePlaneIndex(self, coordinates, z):
        v = self.getZVector(z)
        v[coordinates[1]] = coordinates[0]
        return self.getZ(v)

    def getHelperPlanesIndexes(self, k):
        x, y = self.getNodeCoordinates(k)
        return [z for z in range(self.subPacketSize) if self.getZVector(z)[y] == x]


class ClayCodeErasureDecodingStep:
    """new ClayCodeErasureDecodingStep(erasedIndexes, RS(2,2), RS(k,m)) (:43-51)."""

    def __init__(self, erasedIndexes, numDataUnits: int, numParityUnits: int, virtualUnits: int = 0,
                 isTest: bool = False):
        """virtualUnits > 0: shortened code, Clay(k+v, m) with v virtual zero data nodes
        (e.g. Clay(10,4) = ClayCodeErasureDecodingStep(e, 10, 4, virtualUnits=2)).  isTest: the
        reference run with -DisTest=true (decodeDecoupledPlane :571-581, ecx_clay_create_ex)."""
        er = np.ascontiguousarray(list(erasedIndexes), np.int32)
        h = ctypes.c_void_p()
        if isTest:
            check(lib().ecx_clay_create_ex(numDataUnits, numParityUnits, virtualUnits, er.ctypes.data, len(er),
                                           1, ctypes.byref(h)))
        elif virtualUnits:
            check(lib().ecx_clay_create_shortened(numDataUnits, numParityUnits, virtualUnits, er.ctypes.data,
                                                  len(er), ctypes.byref(h)))
        else:
            check(lib().ecx_clay_create(numDataUnits, numParityUnits, er.ctypes.data, len(er), ctypes.byref(h)))
        self.isTest = isTest
        self._h = h
        self.erasedIndexes = list(erasedIndexes)
        self.numDataUnits, self.numParityUnits = numDataUnits, numParityUnits
        self.numTotalUnits = numDataUnits + numParityUnits
        q, t, a = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().ecx_clay_geometry(h, ctypes.byref(q), ctypes.byref(t), ctypes.byref(a)))
        self.q, self.t, self.subPacketSize = q.value, t.value, a.value
        self.virtualUnits = virtualUnits
        self.util = ClayCodeUtil(erasedIndexes, numDataUnits + virtualUnits, numParityUnits)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().ecx_clay_destroy(self._h)
            self._h = None

    def rtcCompileCheck(self) -> int:
        """Build this single-node repair's per-helper-plane program (checked against the
        composed reference map), generate its kernel and compile it with hiprtc for
        gfx950; returns the code-object size (ecx_clay_rtc_compile_check, include/ecx_tune.h)."""
        f = lib().ecx_clay_rtc_compile_check
        f.argtypes, f.restype = [ctypes.c_void_p], ctypes.c_int
        return check(f(self._h))

    def rtcSource(self) -> str:
        """The generated k_clay_repair source (ecx_clay_rtc_source)."""
        f = lib().ecx_clay_rtc_source
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int], ctypes.c_int
        n = check(f(self._h, None, 0))
        buf = ctypes.create_string_buffer(n + 1)
        check(f(self._h, buf, n + 1))
        return buf.value.decode()

    def getHelperPlanesIndexes(self, erasedIndex: int):
        out = np.zeros(self.subPacketSize, np.int32)
        n = check(lib().ecx_clay_helper_planes(self._h, erasedIndex, out.ctypes.data))
        return [int(x) for x in out[:n]]

    def performCoding(self, inputs, outputs, bufSize: Optional[int] = None) -> None:
        """inputs: n*alpha (plane-major, None = absent); outputs: |E|*alpha arrays.
        Entries may be numpy arrays, None, ECChunk or ECBlock (ECChunk.toBuffers)."""
        inputs, outputs = _buffers(inputs), _buffers(outputs)
        if len(inputs) != self.numTotalUnits * self.subPacketSize:
            raise EcxError(-1, "Invalid inputs length")
        if len(outputs) != len(self.erasedIndexes) * self.subPacketSize:
            raise EcxError(-1, "Invalid outputs length")
        if bufSize is None:
            first = next((b for b in inputs if b is not None), None)
            if first is None:
                raise EcxError(-1, "Invalid inputs are found, all being null")
            bufSize = len(first)
        check(lib().ecx_clay_perform_coding(self._h, _ptr_array(inputs), _ptr_array(outputs), bufSize))

    def doDecodeSingleHelper(self, helperCoupledPlanes, helperIndex: int, outputs, erasedIndex: int,
                             bufSize: int) -> None:
        """doDecodeSingle overload 2 (:225-282): helperCoupledPlanes[nh][n], outputs[alpha]."""
        flat = [b for row in helperCoupledPlanes for b in row]
        check(lib().ecx_clay_decode_single_helper(self._h, _ptr_array(flat), helperIndex, _ptr_array(outputs),
                                                  erasedIndex, bufSize))

    def map(self) -> GfMap:
        h = ctypes.c_void_p()
        check(lib().ecx_clay_map(self._h, ctypes.byref(h)))
        return GfMap(h, owner=self)

    def _check_batch(self, inp, iss, isl, out, oss, osl, nstripes, nbytes):
        if not self.erasedIndexes:
            return
        if getattr(self, "_map", None) is None:
            self._map = self.map()
        self._map._check(inp, iss, isl, out, oss, osl, nstripes, nbytes)

    def performCodingBatch(self, inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride,
                           nstripes, bufSize, stream=None) -> None:
        self._check_batch(inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride, nstripes,
                          bufSize)
        check(lib().ecx_clay_perform_coding_batch(self._h, _dev_ptr(inp), in_stripe_stride, in_sub_stride,
                                                  _dev_ptr(out), out_stripe_stride, out_sub_stride, nstripes,
                                                  bufSize, _stream(stream)))

    def performCodingBatchHost(self, inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride,
                               nstripes, bufSize) -> None:
        """performCodingBatch over host-memory stripes (ecx_clay_perform_coding_batch_host)."""
        self._check_batch(inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride, nstripes,
                          bufSize)
        check(lib().ecx_clay_perform_coding_batch_host(self._h, _host_ptr(inp), in_stripe_stride, in_sub_stride,
                                                       _host_ptr(out), out_stripe_stride, out_sub_stride, nstripes,
                                                       bufSize))

    def performCodingBatchHostDevices(self, inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride,
                                      out_sub_stride, nstripes, bufSize, devices) -> None:
        """performCodingBatchHost split over several GPUs of this process
        (ecx_clay_perform_coding_batch_host_devices): contiguous stripe ranges (byte ranges of
        every sub-chunk when there are fewer stripes than entries), one worker thread and pipe per
        device entry."""
        self._check_batch(inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride, nstripes,
                          bufSize)
        devs = list(devices)
        arr = np.ascontiguousarray(devs + [0], np.int32)  # never a null list: an empty one is ndev 0
        check(lib().ecx_clay_perform_coding_batch_host_devices(self._h, _host_ptr(inp), in_stripe_stride,
                                                               in_sub_stride, _host_ptr(out), out_stripe_stride,
                                                               out_sub_stride, nstripes, bufSize, arr.ctypes.data,
                                                               len(devs)))


class ClayParityCheck:
    """isParityCorrect for Clay stripes (ecx_clay_is_parity_correct_batch): whether each stripe of a
    device-resident batch is still a codeword of Clay(dataUnits, parityUnits) -- shortened by
    ``virtualUnits`` zero data nodes -- in one read-only launch.  A codeword test: a failing stripe's
    verdict does not say which node is corrupt."""

    def __init__(self, dataUnits: int, parityUnits: int, virtualUnits: int = 0):
        self.dataUnits, self.parityUnits, self.virtualUnits = int(dataUnits), int(parityUnits), int(virtualUnits)
        # The handle is kept until close() / __del__: it holds the shared codec, and with it the proved
        # check program and its device records, which the kernel nodes of a captured call point to.
        self._h = None
        h = ctypes.c_void_p()
        check(lib().ecx_clay_create_shortened(self.dataUnits, self.parityUnits, self.virtualUnits, None, 0,
                                              ctypes.byref(h)))
        self._h = h
        q, t, a = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().ecx_clay_geometry(h, ctypes.byref(q), ctypes.byref(t), ctypes.byref(a)))
        self._geometry = (q.value, t.value, a.value, self.dataUnits + self.parityUnits)

    def close(self) -> None:
        """Release the codec reference; idempotent.  Not while enqueued work is in flight, and not
        before a graph that captured isParityCorrectBatch is destroyed."""
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            lib().ecx_clay_destroy(h)

    def __del__(self):
        self.close()

    def geometry(self):
        """(q, t, alpha, n_real): a stripe holds alpha * n_real sub-chunks, real slot z * n_real + node."""
        return self._geometry

    def isParityCorrectBatch(self, stripes, stripe_stride, sub_stride, nstripes, bufSize, verdict, stream=None) -> None:
        """Over nstripes device-resident stripes in performCodingBatch's input layout (real slot
        z * n_real + node of stripe s at s * stripe_stride + slot * sub_stride, bufSize bytes each):
        the device uint8 array ``verdict`` (nstripes bytes) receives 1 for each stripe that is a
        codeword over [0, bufSize) of every sub-chunk, else 0.  Enqueued on ``stream``; read verdict
        after synchronising.  The first call of a geometry on a device must be outside stream capture;
        keep this object alive as long as a graph that captured the call."""
        if not self._h:
            raise EcxError(-1, "ClayParityCheck is closed")
        _, _, alpha, n_real = self._geometry
        _check_layout(stripes, stripe_stride, sub_stride, alpha * n_real - 1, nstripes, bufSize, "stripes")
        _check_layout(verdict, 1, 0, 0, nstripes, 1, "verdict")
        check(lib().ecx_clay_is_parity_correct_batch(self.dataUnits, self.parityUnits, self.virtualUnits,
                                                     _dev_ptr(stripes), stripe_stride, sub_stride, nstripes, bufSize,
                                                     _dev_ptr(verdict), _stream(stream)))


class ClayPatternSet:
    """ecx_clay_pattern_set: up to 256 erased-node lists of one Clay geometry as one device plan,
    for performCoding (ClayCodeErasureDecodingStep.java:53-107) over a batch whose stripes lost
    different nodes.  List p is ``ClayCodeErasureDecodingStep(erasedLists[p], ...)``'s repair: input
    slot z*n + node, output slot z*len(erasedLists[p]) + j.  An empty list does nothing.  close()
    (idempotent) frees the set."""

    def __init__(self, erasedLists, numDataUnits: int, numParityUnits: int, virtualUnits: int = 0):
        lists = [[int(e) for e in lst] for lst in erasedLists]
        flat = np.ascontiguousarray([e for lst in lists for e in lst] + [0], np.int32)  # never a null array
        counts = np.ascontiguousarray([len(lst) for lst in lists] + [0], np.int32)
        h = ctypes.c_void_p()
        self._h = None
        check(lib().ecx_clay_pattern_set_create(numDataUnits, numParityUnits, virtualUnits, flat.ctypes.data,
                                                counts.ctypes.data, len(lists), ctypes.byref(h)))
        self._h = h
        self.erasedLists = lists
        _, self.numTotalUnits, self.subPacketSize, self.maxErased = self.info()

    def info(self):
        """(lists, nodes per stripe, alpha, most nodes any list erases)."""
        if self._h is None:
            raise EcxError(-6, "the pattern set is closed")
        v = [ctypes.c_int() for _ in range(4)]
        check(lib().ecx_clay_pattern_set_info(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def host_plan(self, in_stripe_stride, in_sub_stride, out_stripe_stride, out_sub_stride, nstripes, bufSize):
        """How performCodingBatchMixedHost would move this batch (ecx_clay_pattern_set_host_plan,
        host-only): a dict of the input slots that go up and the output slots that come back per
        stripe, the stripes per chunk, the chunk count, the buffer sets and the copies per chunk."""
        if self._h is None:
            raise EcxError(-6, "the pattern set is closed")
        out = np.zeros(7, np.int64)
        check(lib().ecx_clay_pattern_set_host_plan(self._h, in_stripe_stride, in_sub_stride, out_stripe_stride,
                                                   out_sub_stride, nstripes, bufSize, out.ctypes.data))
        keys = ("slots_up", "slots_down", "chunk", "chunks", "buffers", "h2d_copies", "d2h_copies")
        return {k: int(v) for k, v in zip(keys, out)}

    def _diag(self, name, argtypes):
        """A diagnostic export beside ecx_clay_rtc_source (include/ecx_tune.h), bound on use."""
        if self._h is None:
            raise EcxError(-6, "the pattern set is closed")
        f = getattr(lib(), name)
        f.argtypes, f.restype = [ctypes.c_void_p] + argtypes, ctypes.c_int
        return f

    @property
    def generated(self) -> bool:
        """True for a generated set: single-node lists of maps of more than 64 rows (Clay(12,4),
        the shortened Clay(10,4)), run by the generated kernel k_clay_repair_set."""
        return check(self._diag("ecx_clay_pattern_set_generated", [])(self._h)) == 1

    def rtcSource(self) -> str:
        """The generated k_clay_repair_set source at the current shape knobs
        (ecx_clay_pattern_set_rtc_source); an EcxError for a composed set."""
        f = self._diag("ecx_clay_pattern_set_rtc_source", [ctypes.c_char_p, ctypes.c_int])
        n = check(f(self._h, None, 0))
        buf = ctypes.create_string_buffer(n + 1)
        check(f(self._h, buf, n + 1))
        return buf.value.decode()

    def rtcCompileCheck(self) -> int:
        """Compile the set kernel with hiprtc for gfx950 (no device needed); returns the
        code-object size (ecx_clay_pattern_set_rtc_compile_check)."""
        return check(self._diag("ecx_clay_pattern_set_rtc_compile_check", [])(self._h))

    def rtcResources(self):
        """The loaded set kernel's resources on the current device, a dict of vgprs, lds_bytes,
        scratch_bytes (hipFuncGetAttribute) and code_bytes (the code object's size); compiles and
        loads the kernel when it is not yet (ecx_clay_pattern_set_rtc_resources)."""
        v, code = [ctypes.c_int() for _ in range(3)], ctypes.c_int64()
        f = self._diag("ecx_clay_pattern_set_rtc_resources",
                       [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.POINTER(ctypes.c_int64)])
        check(f(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(code)))
        return {"vgprs": v[0].value, "lds_bytes": v[1].value, "scratch_bytes": v[2].value, "code_bytes": code.value}

    def _check_batch(self, inp, iss, isl, out, oss, osl, nstripes, nbytes):
        if self._h is None:
            raise EcxError(-6, "the pattern set is closed")
        if self.maxErased == 0:
            return
        _check_layout(inp, iss, isl, self.numTotalUnits * self.subPacketSize - 1, nstripes, nbytes, "input")
        _check_layout(out, oss, osl, self.maxErased * self.subPacketSize - 1, nstripes, nbytes, "output")

    def performCodingBatchMixed(self, inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride,
                                ids, nstripes, bufSize, stream=None) -> None:
        """performCodingBatch with a list per stripe, in one launch
        (ecx_clay_perform_coding_batch_mixed): stripe s is repaired with list ``ids[s]`` (a device
        uint8 tensor of nstripes) into output slots 0 .. len(list)*alpha - 1; everything else of
        ``out`` is left untouched.  Only enqueues."""
        self._check_batch(inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride, nstripes,
                          bufSize)
        _check_extent(ids, nstripes, "ids")
        check(lib().ecx_clay_perform_coding_batch_mixed(self._h, _dev_ptr(ids), _dev_ptr(inp), in_stripe_stride,
                                                        in_sub_stride, _dev_ptr(out), out_stripe_stride,
                                                        out_sub_stride, nstripes, bufSize, _stream(stream)))

    def performCodingBatchMixedHost(self, inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride,
                                    out_sub_stride, ids, nstripes, bufSize) -> None:
        """performCodingBatchMixed over host memory, synchronous
        (ecx_clay_perform_coding_mixed_batch_host).  Output slots 0 .. maxErased*alpha - 1 come back
        for every stripe; the part a stripe's own list does not write comes back as zeros."""
        self._check_batch(inp, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride, nstripes,
                          bufSize)
        _check_extent(ids, nstripes, "ids")
        check(lib().ecx_clay_perform_coding_mixed_batch_host(self._h, _host_ptr(ids), _host_ptr(inp),
                                                             in_stripe_stride, in_sub_stride, _host_ptr(out),
                                                             out_stripe_stride, out_sub_stride, nstripes, bufSize))

    def partialBatchMixed(self, ids, nodeOfStripe, inp, in_stripe_stride, in_node_stride, in_sub_stride, acc,
                          acc_stripe_stride, acc_sub_stride, nstripes, bufSize, is_first, stream=None) -> None:
        """One hop of the pipelined repair chain with a list and a helper node per stripe, in one
        launch (ecx_clay_partial_batch_mixed): stripe s adds node ``nodeOfStripe[s]``'s share of list
        ``ids[s]``'s repair to rows 0 .. len(list)*alpha - 1 of ``acc`` (assigns them when
        ``is_first``); both are device uint8 tensors of nstripes.  Plane z of the stripe's node lies
        at ``inp + s * in_stripe_stride + nodeOfStripe[s] * in_node_stride + z * in_sub_stride``
        (in_node_stride 0: this helper's own sub-chunks back to back).  An id without a list, an
        empty list or a node byte that is no node leaves its stripe untouched; so do the rows past a
        list's own.  Only enqueues."""
        if self._h is None:
            raise EcxError(-6, "the pattern set is closed")
        self.refusePartial()
        if self.maxErased != 0 and nstripes > 0 and bufSize > 0:
            if in_node_stride < 0:
                raise EcxError(-1, "input: negative stride")
            _check_layout(inp, in_stripe_stride, in_sub_stride, self.subPacketSize - 1, nstripes,
                          (self.numTotalUnits - 1) * in_node_stride + bufSize, "input")
            _check_layout(acc, acc_stripe_stride, acc_sub_stride, self.maxErased * self.subPacketSize - 1, nstripes,
                          bufSize, "acc")
            _check_extent(ids, nstripes, "ids")
            _check_extent(nodeOfStripe, nstripes, "nodeOfStripe")
        check(lib().ecx_clay_partial_batch_mixed(self._h, _dev_ptr(ids), _dev_ptr(nodeOfStripe), _dev_ptr(inp),
                                                 in_stripe_stride, in_node_stride, in_sub_stride, _dev_ptr(acc),
                                                 acc_stripe_stride, acc_sub_stride, nstripes, bufSize,
                                                 1 if is_first else 0, _stream(stream)))

    def refusePartial(self) -> None:
        """A generated set has no partial-sum hop yet: raises the library's own refusal
        (ecx_clay_partial_batch_mixed, before any device work); nothing for a composed set."""
        if self.generated:
            check(lib().ecx_clay_partial_batch_mixed(self._h, None, None, None, 0, 0, 0, None, 0, 0, 0, 0, 0, None))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().ecx_clay_pattern_set_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def index_erased(lists_per_stripe, cap: int = 256):
    """(lists, ids) of per-stripe erased-node lists: the distinct lists in order of first
    appearance (as tuples; the order of a list's nodes matters, as erasedIndexes does) and, as a
    uint8 array, for each stripe the index of its list among them -- the inputs of ClayPatternSet
    and, once on the device, of performCodingBatchMixed."""
    index, ids = {}, np.zeros(len(lists_per_stripe), np.uint8)
    for s, lst in enumerate(lists_per_stripe):
        key = tuple(int(e) for e in lst)
        if key not in index:
            if len(index) >= min(cap, 256):
                raise EcxError(-1, "more than %d distinct erased-node lists" % min(cap, 256))
            index[key] = len(index)
        ids[s] = index[key]
    return list(index), ids


class JavaRandom:
    """java.util.Random (JDK specification), for ClayCode.getInputs."""

    def __init__(self, seed: int):
        self.seed = (seed ^ 0x5DEECE66D) & ((1 << 48) - 1)

    def _next(self, bits):
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        r = self.seed >> (48 - bits)
        return r - (1 << bits) if r >= 1 << (bits - 1) else r

    def nextInt(self):
        return self._next(32)

    def nextBytes(self, n: int) -> np.ndarray:
        out = np.zeros(n, np.uint8)
        i = 0
        while i < n:
            rnd = self.nextInt() & 0xFFFFFFFF
            for _ in range(min(4, n - i)):
                out[i] = rnd & 0xFF
                rnd >>= 8
                i += 1
        return out


class ClayCode:
    """ClayCode.java facade: RS(2,2) pair transform + RS(k,m) per plane.
    Buffers are numpy arrays inside ECChunk/ECBlock wrappers, as in the reference."""

    def __init__(self, numDataUnits, numParityUnits, blockSize, erasedIndexes):
        self.numDataUnits, self.numParityUnits, self.blockSize = numDataUnits, numParityUnits, blockSize
        self.erasedIndexes = list(erasedIndexes)
        self.erasureDecodingStep = ClayCodeErasureDecodingStep(erasedIndexes, numDataUnits, numParityUnits)
        self.clayCodeUtil = ClayCodeUtil(erasedIndexes, numDataUnits, numParityUnits)

    def performCoding(self, inputs, outputs):
        """ClayCode.performCoding (:43-45) -> ClayCodeErasureDecodingStep.performCoding."""
        self.erasureDecodingStep.performCoding(inputs, outputs, self.blockSize)

    def getInputs(self):
        """ClayCode.getInputs (ClayCode.java:47-77): one Random(123456), nextBytes per data
        sub-chunk in flat order k; sub-chunk k is data iff k % n < numDataUnits."""
        n = self.numDataUnits + self.numParityUnits
        a = self.clayCodeUtil.getSubPacketSize()
        r = JavaRandom(123456)
        out = [None] * (n * a)
        counter = 0
        for i in range(n):
            for j in range(a):
                k = i * a + j
                if counter < self.numDataUnits:
                    out[k] = ECBlock(ECChunk(r.nextBytes(self.blockSize)), False, False)
                else:
                    out[k] = ECBlock(ECChunk(None), True, True)
                counter = (counter + 1) % n
        return out

    def getOutputs(self):
        """ClayCode.getOutputs (:79-87)."""
        return [ECBlock(ECChunk(np.zeros(self.blockSize, np.uint8)), True, True)
                for _ in range(len(self.erasedIndexes) * self.clayCodeUtil.getSubPacketSize())]

    def encode(self, inputs, outputs):
        """ClayCode.encode (:89-99): performCoding with erasedIndexes = the parity nodes;
        returns [inputChunks, outputChunks]."""
        step = ClayCodeErasureDecodingStep(self.erasedIndexes, self.numDataUnits, self.numParityUnits)
        ic, oc = self.getChunks(inputs), self.getChunks(outputs)
        step.performCoding(ic, oc, self.blockSize)
        return [ic, oc]

    def getChunks(self, blocks):
        """ClayCode.getChunks (:168-177)."""
        return [None if b is None else b.getChunk() for b in blocks]

    def getTestOutputs(self, erasedIndexesSize: int):
        """ClayCode.getTestOutputs (:157-166)."""
        return [ECBlock(ECChunk(np.zeros(self.blockSize, np.uint8)), False, True)
                for _ in range(erasedIndexesSize * self.clayCodeUtil.getSubPacketSize())]

    def getTestInputs(self, inputChunks, outputChunks, testErasedIndexes, blockId: str = "LP", write_dir=None):
        """ClayCode.getTestInputs (:101-155), restated faithfully -- including the
        reference's index quirk (SURVEY.md A.2 bug B1): the outer loop variable is
        treated as the node although the flat index a*alpha+b is plane-major, so
        the zeroed sub-chunks are not the erased node's for every e.  With
        write_dir, also writes the per-sub-chunk files "<blockId> <node> <plane>"
        (and "ORIGINAL ..." for erased nodes) as the reference does in its CWD."""
        n = self.numDataUnits + self.numParityUnits
        a = self.clayCodeUtil.getSubPacketSize()
        erased = list(testErasedIndexes)
        ib, ob = ECChunk.toBuffers(inputChunks), ECChunk.toBuffers(outputChunks)
        test, k = [None] * (n * a), 0
        for aa in range(n):
            for b in range(a):
                i = aa * a + b
                if aa not in erased:
                    if ib[i] is not None:
                        buf = np.array(ib[i], np.uint8)
                    else:
                        buf = np.array(ob[k], np.uint8)
                        k += 1
                    test[i] = ECBlock(ECChunk(buf), False, True)
                else:
                    if ib[i] is None:
                        k += 1
                    test[i] = ECBlock(ECChunk(np.zeros(self.blockSize, np.uint8)), False, True)
        if write_dir is not None:
            k = 0
            for i in range(a):
                for j in range(n):
                    idx = i * n + j
                    data = ib[idx] if ib[idx] is not None else ob[k]
                    if ib[idx] is None:
                        k += 1
                    write_subchunk(write_dir, blockId, j, i, data, original=j in erased)
        return test


class ClayCodeHelper:
    """ClayCodeHelper.kt:11-76 -- coordinator-side single repair, one helper plane at a time
    (doDecodeSingle overload 2)."""

    def __init__(self, NUM_DATA_UNITS, NUM_PARITY_UNITS, SUBPACKET_SIZE, inputs):
        self.k, self.m, self.alpha = NUM_DATA_UNITS, NUM_PARITY_UNITS, SUBPACKET_SIZE
        self.n = NUM_DATA_UNITS + NUM_PARITY_UNITS
        self.inputs = _buffers(inputs)

    def getHelperPlanesAndDecode(self, util, blockId, outputs, erasedIndex, bufSize, isDirect=False):
        """outputs: [alpha][|E|] arrays (|E| = 1)."""
        step = ClayCodeErasureDecodingStep([erasedIndex], self.k, self.m)
        hidx = util.getHelperPlanesIndexes(erasedIndex)
        rows = [[self.inputs[z * self.n + j] for j in range(self.n)] for z in hidx]
        flat_out = [outputs[z][0] for z in range(self.alpha)]
        for i in range(len(hidx)):
            step.doDecodeSingleHelper(rows, i, flat_out, erasedIndex, bufSize)


# ---------------------------------------------------------------- per-sub-chunk files
def _subchunk_path(directory, blockId, node, plane, original=False):
    import os
    return os.path.join(str(directory), f"{'ORIGINAL ' if original else ''}{blockId} {node} {plane}")


def write_subchunk(directory, blockId: str, node: int, plane: int, data, original: bool = False) -> str:
    """The reference's on-disk unit: one file "<blockId> <node> <plane>" holding exactly
    B bytes (ClayCode.java:140-152, ClayCodeNode.kt:105,147,245,257)."""
    path = _subchunk_path(directory, blockId, node, plane, original)
    np.asarray(data, np.uint8).tofile(path)
    return path


def read_subchunk(directory, blockId: str, node: int, plane: int, blockSize: Optional[int] = None,
                  original: bool = False) -> np.ndarray:
    data = np.fromfile(_subchunk_path(directory, blockId, node, plane, original), dtype=np.uint8)
    return data if blockSize is None else data[:blockSize].copy()


# ---------------------------------------------------------------- LRC (lrc/)
class LRCErasureUtil:
    N = 16
    K = 12
    R = 3


class LRCErasureCode:
    """LRCErasureCode.kt:5-9 -- RS(R,1) local parity (coefficients [1,1,1]: XOR)."""

    def __init__(self):
        self.rs = ReedSolomon.create(LRCErasureUtil.R, 1)

    def encodeParitySingle(self, shard, output, index, blockSize):
        self.rs.encodeParitySingle(shard, output, index, 0, 0, blockSize)

    @staticmethod
    def map(blockPresent=None) -> GfMap:
        """The composed LRC map over the 16 blocks: encode (None) or decode (ecx_lrc_map)."""
        h = ctypes.c_void_p()
        pres = None if blockPresent is None else np.array([1 if p else 0 for p in blockPresent], np.uint8)
        check(lib().ecx_lrc_map(None if pres is None else pres.ctypes.data, ctypes.byref(h)))
        return GfMap(h)

    @staticmethod
    def encodeBatch(stripes, stripe_stride, block_stride, nstripes, blockSize, stream=None) -> None:
        """All group parities of device-resident [S][16][B] stripes, in place (ecx_lrc_encode_batch)."""
        LRCErasureCode.map()._check(stripes, stripe_stride, block_stride, stripes, stripe_stride, block_stride,
                                    nstripes, blockSize)
        check(lib().ecx_lrc_encode_batch(_dev_ptr(stripes), stripe_stride, block_stride, nstripes, blockSize,
                                         _stream(stream)))

    @staticmethod
    def decodeBatch(stripes, stripe_stride, block_stride, blockPresent, nstripes, blockSize, stream=None) -> None:
        """Rebuild the non-present blocks of device-resident stripes in place (ecx_lrc_decode_batch)."""
        pres = np.array([1 if p else 0 for p in blockPresent], np.uint8)
        if pres.all():
            return
        LRCErasureCode.map(blockPresent)._check(stripes, stripe_stride, block_stride, stripes, stripe_stride,
                                                block_stride, nstripes, blockSize)
        check(lib().ecx_lrc_decode_batch(_dev_ptr(stripes), stripe_stride, block_stride, pres.ctypes.data, nstripes,
                                         blockSize, _stream(stream)))


def lrc_encode(data: np.ndarray):
    """LRCErasureCodeExample.encode (:30-57): K blocks -> N blocks (group g: 3 data + parity)."""
    U = LRCErasureUtil
    block = len(data) // U.K
    rs = ReedSolomon.create(U.R, 1)
    out, pos = [], 0
    for _ in range(U.K // U.R):
        shards = []
        for _ in range(U.R):
            shards.append(np.ascontiguousarray(data[pos:pos + block], np.uint8).copy())
            pos += block
        shards.append(np.zeros(block, np.uint8))
        rs.encodeParity(shards, 0, block)
        out.extend(shards)
    return out


def lrc_encode_using_single(data: np.ndarray):
    """LRCErasureCodeExample.encodeUsingSingle (:59-90)."""
    U = LRCErasureUtil
    block = len(data) // U.K
    code = LRCErasureCode()
    out, pos = [], 0
    for _ in range(U.K // U.R):
        shards = []
        for _ in range(U.R):
            shards.append(np.ascontiguousarray(data[pos:pos + block], np.uint8).copy())
            pos += block
        acc = np.zeros(block, np.uint8)
        for idx in range(U.R):
            code.rs.encodeParitySingle(shards[idx], acc, idx, 0, 0, block)
        shards.append(acc)
        out.extend(shards)
    return out


def lrc_decode(blocks, missingIndices: Iterable[int], blockSize: int):
    """LRCErasureCodeExample.decode (:92-131): returns (file bytes, repaired blocks)."""
    U = LRCErasureUtil
    missing = set(missingIndices)
    rs = ReedSolomon.create(U.R, 1)
    shards = [np.array(blocks[i], np.uint8) if (i not in missing and blocks[i] is not None)
              else np.zeros(blockSize, np.uint8) for i in range(U.N)]
    for g in range(U.K // U.R):
        lo = g * (U.R + 1)
        present = [(lo + j) not in missing for j in range(U.R + 1)]
        rs.decodeMissing(shards[lo:lo + U.R + 1], present, 0, blockSize)
    data = [shards[i] for i in range(U.N) if i == 0 or (i + 1) % (U.R + 1) != 0]
    return np.concatenate(data), shards


# ---------------------------------------------------------------- SampleEncoder / SampleDecoder
def sample_encode(file_bytes: np.ndarray, data_shards: int = 4, parity_shards: int = 2):
    """SampleEncoder.java:54-83: [int32 BE length][file][zero pad] -> data shards + RS parity."""
    size = len(file_bytes)
    shard = (size + 4 + data_shards - 1) // data_shards
    allb = np.zeros(shard * data_shards, np.uint8)
    allb[:4] = np.frombuffer(int(size).to_bytes(4, "big"), np.uint8)
    allb[4:4 + size] = file_bytes
    shards = [allb[i * shard:(i + 1) * shard].copy() for i in range(data_shards)]
    shards += [np.zeros(shard, np.uint8) for _ in range(parity_shards)]
    ReedSolomon.create(data_shards, parity_shards).encodeParity(shards, 0, shard)
    return shards


def sample_decode(shards: Sequence[Optional[np.ndarray]], data_shards: int = 4, parity_shards: int = 2):
    """SampleDecoder.java:34-98: decodeMissing, then strip the length header."""
    present = [s is not None for s in shards]
    if sum(present) < data_shards:
        raise EcxError(-2, "Not enough shards present")
    size = next(len(s) for s in shards if s is not None)
    work = [np.array(s, np.uint8) if s is not None else np.zeros(size, np.uint8) for s in shards]
    ReedSolomon.create(data_shards, parity_shards).decodeMissing(work, present, 0, size)
    allb = np.concatenate(work[:data_shards])
    n = int.from_bytes(allb[:4].tobytes(), "big")
    return allb[4:4 + n].copy(), work
