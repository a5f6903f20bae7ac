"""Host-side mirror of the reference's aggregation interface, over the C-ABI.

The reference keeps the aggregator state in static maps (PeerData.java:137-189)
and reduces inside IPLS / Updater methods.  ``Aggregator`` owns the same state
on one GPU (one ``ipls_agg`` handle) and exposes the reference's operations
under the reference's names, with the reference's argument meaning:

=====================================  =========================================
reference (src/main/java/)             here
=====================================  =========================================
IPLS.InitializeWeights(List) 1880      ``InitializeWeights(model)``
IPLS.OrganizeGradients 1018            ``OrganizeGradients(gradients)``
IPLS.UpdateGradient 1703 (1737-1743)   ``UpdateGradient(gradients, auth_list)``
Updater._Update 31 (from_clients)      ``Update(gradient, partition, from_clients)``
Download_Scheduler 245-268             ``OtherReplicaGradients(p, aggregator, g)``
IPLS.Collect_Replicas 1217             ``Collect_Replicas()``
IPLS.Update_Client_WaitAck_List 1556   ``PromoteFuture(auth_list)``
Updater.run indirect 176-187           ``UpdateIndirect(file_bytes, partition)``
Decentralized_Storage_Receiver 239     ``Merge(partition, buckets)``
IPLS.AggregatePartition 1248           ``AggregatePartition(partition)``
Download_Scheduler.cache_partition 752 ``cache_partition(partition, data)``
IPLS.GetPartitions 1080 (1140-1174)    ``GetPartitions()``
=====================================  =========================================

Host buffers are numpy arrays (``float64`` for doubles, ``uint8``/bytes for the
big-endian IPFS file format and pubsub frames).  Device buffers may be passed
as ``DeviceBuffer`` (raw pointer + length) -- e.g. ``torch`` CUDA tensors via
``DeviceBuffer.from_tensor``.  Every call goes to the HIP library; a missing
library raises at construction.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _native as N


@dataclass
class DeviceBuffer:
    """A device-resident operand: address, element count, big-endian or not.

    ``dtype`` is ``"f64"`` (doubles, or big-endian double bytes), ``"f32"``
    (a trainer's float parameters or gradients, Model.java:423 / 388-390: the
    library widens or narrows them on the device), ``"half"`` (IEEE binary16)
    or ``"bf16"`` (bfloat16) -- what a trainer under autocast holds; ``n``
    counts elements of that dtype.  Only f64 buffers can be big-endian.

    The handle's HIP stream is non-blocking (include/ipls_agg.h): bytes
    written by torch or the null stream must be complete before the call
    that reads them (``torch.cuda.synchronize()``, or an event the handle's
    stream ``Aggregator.stream`` waits on)."""
    ptr: int
    n: int
    big_endian: bool = False
    dtype: str = "f64"

    def __post_init__(self):
        if self.dtype not in ("f64", "f32", "half", "bf16"):
            raise ValueError(f"dtype must be 'f64', 'f32', 'half' or 'bf16', not {self.dtype!r}")
        if self.dtype != "f64" and self.big_endian:
            raise ValueError(f"big-endian buffers hold doubles: dtype={self.dtype!r} cannot be big_endian")

    @classmethod
    def from_tensor(cls, t, big_endian: bool = False) -> "DeviceBuffer":
        """A ``torch.float32`` tensor gives an f32 buffer, a ``torch.float16``
        one a ``"half"`` buffer and a ``torch.bfloat16`` one a ``"bf16"``
        buffer, each of ``numel()`` elements; every other dtype is a carrier
        of 8-byte values (float64, or uint8 / int64 holding doubles or
        big-endian double bytes).  The two 16-bit dtypes used to be read as
        such carriers (``numel() * 2 // 8`` "doubles"), which could only ever
        produce garbage; they are now the values they hold."""
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("need a contiguous device tensor")
        trainer = _TORCH_DTYPES.get(str(t.dtype))
        if trainer is not None:
            return cls(int(t.data_ptr()), t.numel(), big_endian, trainer)
        return cls(int(t.data_ptr()), t.numel() * t.element_size() // 8, big_endian)

    @property
    def kind(self) -> int:
        if self.dtype != "f64":
            return _DEV_KIND[self.dtype]
        return N.DEV_BE if self.big_endian else N.DEV_F64


# the trainer dtypes (widened / narrowed on the device): torch dtype -> name,
# name -> DEV kind, HOST kind, element noun of the error messages
_TORCH_DTYPES = {"torch.float32": "f32", "torch.float16": "half", "torch.bfloat16": "bf16"}
_DEV_KIND = {"f32": N.DEV_F32, "half": N.DEV_F16, "bf16": N.DEV_BF16}
_HOST_KIND = {"f32": N.HOST_F32, "half": N.HOST_F16, "bf16": N.HOST_BF16}
_NOUN = {"f64": "doubles", "f32": "floats", "half": "halves", "bf16": "bfloat16s"}


_SEG_KIND = {"torch.float64": N.DEV_F64, "torch.float32": N.DEV_F32, "torch.float16": N.DEV_F16,
             "torch.bfloat16": N.DEV_BF16}


class Segments:
    """A flat vector given as a LIST of device tensors (a model's parameters,
    or their gradients): the concatenation of the tensors in list order, each
    read in memory order -- ``parameters_to_vector`` order -- without the
    ``torch.cat`` that would build it or the copy-out that would scatter it
    (include/ipls_agg.h, the ``_segs`` calls).  ``from_tensors`` builds the
    three tables the library takes once; the object keeps the tensors alive
    and can be passed again every step.  ``n`` is the number of values,
    ``n_segs`` the number of tensors, ``tensors`` the tuple itself.  As with
    DeviceBuffer, what torch wrote must be complete before the call."""

    def __init__(self, tensors, ptrs, ns, kinds):
        self.tensors, self._ptrs, self._ns, self._kinds = tensors, ptrs, ns, kinds
        self.n_segs = len(tensors)
        self.n = int(sum(ns))

    @classmethod
    def from_tensors(cls, tensors) -> "Segments":
        """Contiguous CUDA tensors of float64 / float32 / float16 / bfloat16,
        mixed freely; ``numel() == 0`` is allowed.  Anything else -- a CPU
        tensor, a non-contiguous one, another dtype -- is a ValueError before
        any library call: no silent copy is made."""
        tensors = tuple(tensors)
        for i, t in enumerate(tensors):
            if not getattr(t, "is_cuda", False):
                raise ValueError(f"tensor {i}: need a CUDA tensor")
            if not t.is_contiguous():
                raise ValueError(f"tensor {i}: need a contiguous tensor (no silent copy is made)")
            if str(t.dtype) not in _SEG_KIND:
                raise ValueError(f"tensor {i}: dtype {t.dtype} is not float64, float32, float16 or bfloat16")
        k = len(tensors)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[int(t.data_ptr()) if t.numel() else None for t in tensors])
        ns = (ctypes.c_int64 * max(k, 1))(*[t.numel() for t in tensors])
        kinds = (ctypes.c_int32 * max(k, 1))(*[_SEG_KIND[str(t.dtype)] for t in tensors])
        return cls(tensors, ptrs, ns, kinds)

    @property
    def tables(self):
        """(ptrs, ns, kinds, n_segs) as the C calls take them."""
        return self._ptrs, self._ns, self._kinds, self.n_segs


class Difference:
    """The trainer's update as the difference of two lists of device tensors,
    ``minuend[s] - subtrahend[s]`` element by element in each pair's own dtype
    (what ``torch.sub`` gives), only the result widened -- the reference's
    ``GetDiff(model.params(), Dumm)`` = ``Dumm.sub(params)`` (Model.java:413:
    ``Difference(received_model, trained_params)``) without the third list a
    ``torch._foreach_sub`` would make (include/ipls_agg.h, the ``_segs_diff``
    calls).  Each argument is a ``Segments`` or a list / tuple of CUDA
    tensors; a single tensor counts as a list of one, so two flat tensors are
    a one-segment difference.  The pairs must agree in number, ``numel()`` and
    dtype, else a ValueError naming the tensor, before any library call.  The
    object keeps both lists alive and can be passed again every step to
    ``UpdateGradient`` and ``SendGradients``; ``n`` is the number of values,
    ``n_segs`` the number of pairs.  The lists may alias."""

    def __init__(self, minuend, subtrahend):
        a, b = self._list(minuend), self._list(subtrahend)
        if a.n_segs != b.n_segs:
            raise ValueError(f"minuend has {a.n_segs} tensors, subtrahend {b.n_segs}")
        for i, (x, y) in enumerate(zip(a.tensors, b.tensors)):
            if x.numel() != y.numel():
                raise ValueError(f"tensor {i}: minuend has {x.numel()} elements, subtrahend {y.numel()}")
            if x.dtype != y.dtype:
                raise ValueError(f"tensor {i}: minuend dtype {x.dtype}, subtrahend dtype {y.dtype}")
        self.minuend, self.subtrahend = a, b
        self.n, self.n_segs = a.n, a.n_segs

    @staticmethod
    def _list(x):
        if isinstance(x, Segments):
            return x
        return Segments.from_tensors(x if isinstance(x, (list, tuple)) else [x])

    @property
    def tables(self):
        """(a_ptrs, b_ptrs, ns, kinds, n_segs) as the C calls take them."""
        a_ptrs, ns, kinds, k = self.minuend.tables
        return a_ptrs, self.subtrahend.tables[0], ns, kinds, k


class PeerUpdates:
    """The updates of K trainers of one architecture, folded by ONE
    ``UpdateGradient`` call in peer order (include/ipls_agg.h,
    ``ipls_agg_update_gradient_segs_peers``; k_update_segs_peers): the
    accumulators end with the bits of K calls, one per peer, each with the
    same ``auth_list``.  ``trained_lists`` holds one list per peer, each a
    ``Segments``, a list / tuple of CUDA tensors or a single tensor.  With
    ``received`` (the model every trainer started from, the same forms) peer
    k's update is ``Difference(received, trained_lists[k])``, the received
    model read once; without it the lists are the updates themselves.  Every
    list must agree with peer 0's (and with ``received``) in number of
    tensors, ``numel()`` and dtype, else a ValueError naming the peer and the
    tensor, before any library call.  The object keeps every tensor alive and
    can be passed again every step; ``n`` is the number of values,
    ``n_segs`` the number of tensors per list, ``n_peers`` the number of
    lists.  The lists may alias."""

    def __init__(self, trained_lists, received=None):
        peers = [Difference._list(x) for x in trained_lists]
        if not 1 <= len(peers) <= N.SEG_PEERS_MAX:
            raise ValueError(f"need 1 to {N.SEG_PEERS_MAX} peers, not {len(peers)}")
        rec = None if received is None else Difference._list(received)
        first = peers[0]
        for name, x in ([("received", rec)] if rec is not None else []) + [(f"peer {k}", p) for k, p in
                                                                           enumerate(peers[1:], 1)]:
            if x.n_segs != first.n_segs:
                raise ValueError(f"{name} has {x.n_segs} tensors, peer 0 has {first.n_segs}")
            for i, (a, b) in enumerate(zip(first.tensors, x.tensors)):
                if a.numel() != b.numel():
                    raise ValueError(f"{name}, tensor {i}: {b.numel()} elements, peer 0 has {a.numel()}")
                if a.dtype != b.dtype:
                    raise ValueError(f"{name}, tensor {i}: dtype {b.dtype}, peer 0 has {a.dtype}")
        self.peers, self.received = tuple(peers), rec
        self.n, self.n_segs, self.n_peers = first.n, first.n_segs, len(peers)
        k = self.n_segs
        self._t_ptrs = (ctypes.c_void_p * max(k * self.n_peers, 1))(*[p.tables[0][s] for p in peers for s in range(k)])

    @property
    def tables(self):
        """(m_ptrs or None, t_ptrs, n_peers, ns, kinds, n_segs) as the C call takes them."""
        _, ns, kinds, k = self.peers[0].tables
        return (None if self.received is None else self.received.tables[0]), self._t_ptrs, self.n_peers, ns, kinds, k

    def outputs(self) -> "ModelCopies":
        """The way back out of the round: the ``ModelCopies`` of ``received``
        (when there is one) followed by the K trained lists, for
        ``GetPartitions(out=...)`` to write the new model into all of them in
        one call."""
        return ModelCopies(([self.received] if self.received is not None else []) + list(self.peers))


class ModelCopies:
    """Several lists of device tensors of one architecture -- the parameter
    tensors of K trainers, and the received model they share -- that ONE
    ``GetPartitions(out=...)`` call writes the averaged model into
    (include/ipls_agg.h, ``ipls_agg_get_partitions_segs_copies``;
    k_divide_segs_copies): every list ends with the bits of
    ``GetPartitions(out=Segments(list))``, W read and divided once, every
    list from the same W.  ``lists`` holds one list per copy, each a
    ``Segments``, a list / tuple of CUDA tensors or a single tensor.  Every
    list must agree with list 0's in number of tensors, ``numel()`` and dtype,
    else a ValueError naming the list and the tensor, before any library call.
    The object keeps every tensor alive and can be passed again every round;
    ``n`` is the number of values, ``n_segs`` the number of tensors per list,
    ``n_lists`` the number of lists.  Lists that overlap are the caller's
    problem."""

    def __init__(self, lists):
        copies = [Difference._list(x) for x in lists]
        if not 1 <= len(copies) <= N.SEG_COPIES_MAX:
            raise ValueError(f"need 1 to {N.SEG_COPIES_MAX} lists, not {len(copies)}")
        first = copies[0]
        for name, x in [(f"list {k}", c) for k, c in enumerate(copies[1:], 1)]:
            if x.n_segs != first.n_segs:
                raise ValueError(f"{name} has {x.n_segs} tensors, list 0 has {first.n_segs}")
            for i, (a, b) in enumerate(zip(first.tensors, x.tensors)):
                if a.numel() != b.numel():
                    raise ValueError(f"{name}, tensor {i}: {b.numel()} elements, list 0 has {a.numel()}")
                if a.dtype != b.dtype:
                    raise ValueError(f"{name}, tensor {i}: dtype {b.dtype}, list 0 has {a.dtype}")
        self.lists = tuple(copies)
        self.n, self.n_segs, self.n_lists = first.n, first.n_segs, len(copies)
        k = self.n_segs
        self._o_ptrs = (ctypes.c_void_p * max(k * self.n_lists, 1))(*[c.tables[0][s] for c in copies for s in range(k)])

    @property
    def tables(self):
        """(o_ptrs, n_lists, ns, kinds, n_segs) as the C call takes them."""
        _, ns, kinds, k = self.lists[0].tables
        return self._o_ptrs, self.n_lists, ns, kinds, k


def _segments(x):
    """x as a Segments when it is one, or a list / tuple of CUDA tensors (wrapped on the fly); else None."""
    if isinstance(x, Segments):
        return x
    if isinstance(x, (list, tuple)) and x and all(getattr(t, "is_cuda", False) for t in x):
        return Segments.from_tensors(x)
    return None


def _out_dtype(dtype):
    """'f64', 'f32', 'half' or 'bf16' for the ``dtype=`` of GetPartitions /
    aggregate_round: a numpy dtype, or the string "bf16" (numpy has no
    bfloat16: the host array then holds the bit patterns as uint16)."""
    if isinstance(dtype, str) and dtype == "bf16":
        return "bf16"
    d = np.dtype(dtype)
    return "f32" if d == np.float32 else "half" if d == np.float16 else "f64"


def _chunked_dtype(dtype):
    """'f32', 'half' or 'bf16' for the ``dtype=`` of UpdateChunked /
    GetPartitionsChunked: np.float32, np.float16 or the string "bf16";
    anything else is a ValueError (before any library call)."""
    if isinstance(dtype, str) and dtype == "bf16":
        return "bf16"
    try:
        d = np.dtype(dtype)
    except TypeError:
        d = None
    if d == np.float32:
        return "f32"
    if d == np.float16:
        return "half"
    raise ValueError(f"dtype must be np.float32, np.float16 or 'bf16' (or None for doubles), not {dtype!r}")


_NP_OUT = {"f64": np.float64, "f32": np.float32, "half": np.float16, "bf16": np.uint16}


def _bucket_table(buckets, lengths, p_first: int):
    """(flat pointer list, k) of a batched call's bucket table, with the checks
    of _bucket_table_kind (lengths in elements, one dtype per table)."""
    return _bucket_table_kind(buckets, lengths, p_first)[:2]


def _bucket_table_kind(buckets, lengths, p_first: int, big_endian: bool = False):
    """(flat pointer list, k, src_kind) of a batched call's bucket table:
    ``buckets[q]`` are the k device buckets of partition ``p_first + q``.  The
    C-ABI takes bare pointers and reads L_p elements from each
    (include/ipls_agg.h), so a DeviceBuffer shorter than its partition -- in
    elements of its dtype -- is refused here, before any launch could read
    past it.  The kind is DEV_F32 / DEV_F16 / DEV_BF16 when the DeviceBuffers
    are f32 / half / bf16 (one call folds one kind: a table that mixes dtypes
    is refused), else DEV_BE / DEV_F64 by ``big_endian``, which applies to f64
    buckets only.
    Raw integer addresses are the caller's contract; partitions out of range
    are left to the library's range check."""
    n_parts = len(buckets)
    k = len(buckets[0]) if n_parts else 0
    flat = []
    dtypes = set()
    for q, row in enumerate(buckets):
        if len(row) != k:
            raise ValueError("every partition needs the same number of buckets")
        p = p_first + q
        need = lengths[p] if 0 <= p < len(lengths) else 0
        for b in row:
            if isinstance(b, DeviceBuffer):
                if b.n < need:
                    raise ValueError(f"partition {p} needs buckets of {need} "
                                     f"{_NOUN[b.dtype]}, a DeviceBuffer holds {b.n}")
                dtypes.add(b.dtype)
                flat.append(b.ptr)
            else:
                flat.append(int(b))
    if len(dtypes) > 1:
        raise ValueError("a bucket table holds DeviceBuffers of one dtype (f64, f32, half or bf16), not a mix")
    if dtypes and dtypes != {"f64"}:
        if big_endian:
            raise ValueError("big_endian applies to f64 buckets only")
        return flat, k, _DEV_KIND[dtypes.pop()]
    return flat, k, (N.DEV_BE if big_endian else N.DEV_F64)


def _host_operand(x, big_endian: bool, f32: bool = False):
    """(pointer, n_elements, kind, keepalive) for a host operand.  ``f32``: the
    call takes the HOST trainer kinds (include/ipls_agg.h), so a numpy float32
    or float16 array, or a contiguous CPU torch.float16 / torch.bfloat16
    tensor, goes as it is (4 or 2 B per element) and is widened on the device;
    elsewhere it is widened here."""
    tdt = str(getattr(x, "dtype", "")) if hasattr(x, "data_ptr") else ""
    if tdt in ("torch.float16", "torch.bfloat16"):   # a CPU tensor (numpy has no bfloat16)
        if f32 and x.is_contiguous() and x.device.type == "cpu":
            return int(x.data_ptr()), x.numel(), _HOST_KIND[_TORCH_DTYPES[tdt]], x
        x = x.double().numpy()
    if isinstance(x, (bytes, bytearray, memoryview)):
        a = np.frombuffer(x, dtype=np.uint8)
    else:
        a = np.asarray(x)
    if a.dtype == np.uint8:          # raw bytes are always BE doubles (IPFS file format)
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a.nbytes // 8, N.HOST_BE, a
    if a.dtype.byteorder == ">":
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a.size, N.HOST_BE, a
    if f32 and a.dtype == np.float32:   # a trainer's floats: 4 B per element to the device, widened there
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a.size, N.HOST_F32, a
    if f32 and a.dtype == np.float16:   # halves: 2 B per element to the device, widened there
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a.size, N.HOST_F16, a
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.ctypes.data, a.size, N.HOST_F64, a


def _operand(x, big_endian: bool = False, f32: bool = False):
    if isinstance(x, Difference):
        raise TypeError("a Difference is an operand of UpdateGradient and SendGradients only")
    if isinstance(x, PeerUpdates):
        raise TypeError("a PeerUpdates is an operand of UpdateGradient only")
    if isinstance(x, ModelCopies):
        raise TypeError("a ModelCopies is an output of GetPartitions only")
    if isinstance(x, DeviceBuffer):
        return x.ptr, x.n, x.kind, x
    return _host_operand(x, big_endian, f32)


def _callback(caught: list, fn, *args) -> int:
    """Body of a chunk source/sink called from C: 0 to go on, 1 to stop.  No
    exception may unwind through the library, so any -- a socket's EOFError
    or timeout, a KeyboardInterrupt -- is kept and stops the call; the Python
    caller re-raises it (_reraise) once the library has returned."""
    if caught:
        return 1
    try:
        return 0 if fn(*args) else 1
    except BaseException as e:   # noqa: BLE001 -- re-raised after the library call
        caught.append(e)
        return 1


def _reraise(caught: list) -> None:
    if caught:
        raise caught[0]


class Aggregator:
    """One aggregator's partition accumulators on one MI355X.

    ``model_size``/``n_partitions`` follow Middleware's ``-pa`` semantics and the
    reference chunk rule (IPLS.java:1019-1028).  ``bucket_len`` (with
    model_size=0) selects the synthetic geometry of SURVEY.md §8: every
    partition ``bucket_len`` doubles including the count slot."""

    def __init__(self, model_size: int = 0, n_partitions: int = 1, *, max_peers: int = 0,
                 partial_aggregation: int = 0, secure: bool = False, device: int = 0,
                 bucket_len: int = 0, devices=None, library=None):
        """``devices``: a list of HIP device ordinals shards the partitions over
        several GPUs in contiguous blocks (cfg.devices, ipls_shard_plan); a
        device may repeat (several shards on one GPU).  ``library``: another
        build of the C-ABI (``ipls._native.load(path)``) for same-process A/B
        runs; default the in-tree library."""
        self._lib = library if library is not None else N.lib()
        devs = None if devices is None else (ctypes.c_int32 * len(devices))(*devices)
        cfg = N.AggCfg(model_size=model_size, n_partitions=n_partitions, max_peers=max_peers,
                       partial_aggregation=partial_aggregation, secure=int(bool(secure)),
                       device=device, flags=0, bucket_len=bucket_len,
                       devices=devs, n_devices=0 if devices is None else len(devices), reserved=0)
        h = ctypes.c_void_p()
        N.check(self._lib.ipls_agg_open(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self._hv = h.value                      # the handle's address, for ipls._fast
        self._fast = N.fast() if library is None else None
        self.model_size = model_size
        self.n_partitions = n_partitions
        self.secure = bool(secure)
        self.device = device if devices is None else devices[0]
        self.devices = [device] if devices is None else list(devices)
        self.lengths = [self.partition_len(p) for p in range(n_partitions)]
        self.offsets = [self.partition_offset(p) for p in range(n_partitions)]
        self.flat_size = max(o + L - 1 for o, L in zip(self.offsets, self.lengths))

    # ---- lifetime ----
    def close(self):
        if getattr(self, "_h", None):
            self._hv = None
            self._lib.ipls_agg_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc >= 0:                                # the per-call fast path (UpdateAsync per arrival)
            return rc
        if self._lib is not N.lib():               # a variant build keeps its own error slot
            msg = self._lib.ipls_agg_last_error(None)
            raise N.IplsError(rc, msg.decode(errors="replace") if msg else "")
        return N.check(rc, self._h)

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return int(self._lib.ipls_agg_stream(self._h) or 0)

    def sync(self):
        self._chk(self._lib.ipls_agg_sync(self._h))

    # ---- geometry (IPLS.java:1019-1028) ----
    def partition_len(self, p: int) -> int:
        v = ctypes.c_int64()
        self._chk(self._lib.ipls_agg_partition_len(self._h, p, ctypes.byref(v)))
        return v.value

    def partition_offset(self, p: int) -> int:
        v = ctypes.c_int64()
        self._chk(self._lib.ipls_agg_partition_offset(self._h, p, ctypes.byref(v)))
        return v.value

    # ---- reference operations ----
    def InitializeWeights(self, model, big_endian: bool = False, *, java_list: bool = False):
        """IPLS.java:1880-1901 (model = List<Double>, or read_file's raw BE
        bytes; ``java_list=True``: the bytes of a Java-serialised
        ArrayList<Double>, what DownloadParameters reads, IPLS.java:567).
        A ``Segments`` (the model as its list of parameter tensors) is
        concatenated as doubles on the device here, in the binding, and loaded
        through the same call: this happens once per run, so it has no list
        form in the C-ABI."""
        if isinstance(model, Segments):
            import torch
            flat = (torch.cat([t.reshape(-1).double() for t in model.tensors]) if model.n_segs
                    else torch.empty(0, dtype=torch.float64, device="cuda"))
            torch.cuda.synchronize(flat.device)
            self._chk(self._lib.ipls_agg_load_model(self._h, int(flat.data_ptr()) or None, flat.numel(), N.DEV_F64))
            return
        if java_list:
            keep = _u8(model)
            ptr, n, kind = keep.ctypes.data, keep.size, N.HOST_DLIST
        else:
            ptr, n, kind, keep = _operand(model, big_endian, f32=True)
        self._chk(self._lib.ipls_agg_load_model(self._h, ptr, n, kind))

    def OrganizeGradients(self, gradients, big_endian_out: bool = False) -> dict[int, np.ndarray]:
        """IPLS.java:1018-1040: {p: double[L_p]} with the count slot 1.0."""
        ptr, n, kind, keep = _operand(gradients, f32=True)
        out = {}
        for p in range(self.n_partitions):
            L = self.lengths[p]
            if big_endian_out:
                buf = np.empty(8 * L, dtype=np.uint8)
                dk = N.HOST_BE
            else:
                buf = np.empty(L, dtype=np.float64)
                dk = N.HOST_F64
            self._chk(self._lib.ipls_agg_split(self._h, ptr, n, kind, p, buf.ctypes.data, dk))
            out[p] = buf
        return out

    def UpdateGradient(self, gradients, auth_list):
        """Own-partition accumulate of IPLS.UpdateGradient (IPLS.java:1737-1743).
        ``gradients=None`` is the "did not train in time" call (no-op).  A
        ``Segments``, or a plain list / tuple of CUDA tensors (the gradients
        as autograd left them, mixed dtypes allowed), is read where the
        tensors lie: no ``torch.cat``, no cast pass."""
        owned = np.ascontiguousarray(np.asarray(list(auth_list), dtype=np.int32))
        if gradients is None:
            return
        if isinstance(gradients, Difference):   # minuend - subtrahend, both read where they lie (k_update_segs_diff)
            self._chk(self._lib.ipls_agg_update_gradient_segs_diff(self._h, *gradients.tables, owned.ctypes.data,
                                                                   len(owned)))
            return
        if isinstance(gradients, PeerUpdates):   # K trainers' lists in peer order, one launch (k_update_segs_peers)
            self._chk(self._lib.ipls_agg_update_gradient_segs_peers(self._h, *gradients.tables, owned.ctypes.data,
                                                                    len(owned)))
            return
        segs = _segments(gradients)
        if segs is not None:   # a list of device tensors, read where they lie (k_update_segs)
            self._chk(self._lib.ipls_agg_update_gradient_segs(self._h, *segs.tables, owned.ctypes.data, len(owned)))
            return
        ptr, n, kind, keep = _operand(gradients, f32=True)
        self._chk(self._lib.ipls_agg_update_gradient(
            self._h, ptr, n, kind, owned.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(owned)))

    def round_peers(self, peers, auth_list, out=None):
        """The many-trainers round in one call (include/ipls_agg.h,
        ``ipls_agg_round_segs_peers``; k_round_segs_peers): the state and the
        bits of ``UpdateGradient(peers, auth_list)``, ``AggregatePartition`` of
        every partition in ``auth_list`` and ``GetPartitions(out=out)``, made
        under one hold of each shard's lock in one launch per shard.
        ``peers`` is a ``PeerUpdates``; ``out`` a ``ModelCopies`` over the
        same table, or ``None`` for ``peers.outputs()``: the trainers'
        tensors (and the received model) take the new model in place.
        Returns ``out``."""
        if not isinstance(peers, PeerUpdates):
            raise TypeError(f"round_peers folds a PeerUpdates, not a {type(peers).__name__}")
        if out is None:
            out = peers.outputs()
        elif not isinstance(out, ModelCopies):
            raise TypeError(f"round_peers writes into a ModelCopies (or None: peers.outputs()), not a {type(out).__name__}")
        first = peers.peers[0]
        if out.n_segs != first.n_segs:
            raise ValueError(f"out has {out.n_segs} tensors per list, the peers have {first.n_segs}")
        for i, (a, b) in enumerate(zip(first.tensors, out.lists[0].tensors)):
            if a.numel() != b.numel():
                raise ValueError(f"out, tensor {i}: {b.numel()} elements, the peers have {a.numel()}")
            if a.dtype != b.dtype:
                raise ValueError(f"out, tensor {i}: dtype {b.dtype}, the peers have {a.dtype}")
        owned = np.ascontiguousarray(np.asarray(list(auth_list), dtype=np.int32))
        m_ptrs, t_ptrs, n_peers, ns, kinds, k = peers.tables
        self._chk(self._lib.ipls_agg_round_segs_peers(self._h, m_ptrs, t_ptrs, n_peers, out.tables[0], out.n_lists, ns,
                                                      kinds, k, owned.ctypes.data, len(owned)))
        return out

    def Update(self, gradient, partition: int, from_clients: bool = True, *, frame: bool = False,
               pair: bool = False, from_future: bool = False):
        """Updater._Update: client buckets fold into Aggregated_Gradients
        (Updater.java:115-117), replica partial sums into Replicas_Gradients
        (Updater.java:40-44), and a client's bucket for a later iteration
        (``from_future=True``) into Aggregated_Gradients_from_future
        (Updater.java:99-101).  ``gradient`` may be doubles, big-endian file
        bytes (GetParameters input), a pubsub frame (``frame=True``) or a
        DeviceBuffer.  ``None`` is a no-op, as in the reference."""
        if gradient is None:
            return
        target = N.TGT_FUTURE if from_future else (N.TGT_AGG if from_clients else N.TGT_REP)
        if frame or pair:       # a pubsub frame / a Java-serialised Pair<Integer,double[]> partial update
            a = np.frombuffer(bytes(gradient), dtype=np.uint8)
            self._chk(self._lib.ipls_agg_accumulate(self._h, partition, target, a.ctypes.data,
                                                    a.size, N.HOST_PAIR if pair else N.HOST_FRAME))
            return
        ptr, n, kind, keep = _operand(gradient, f32=True)
        if self._fast is not None:
            rc = self._fast.accumulate(self._hv, partition, target, ptr, n, kind)
            if rc < 0:
                self._chk(rc)
            return
        self._chk(self._lib.ipls_agg_accumulate(self._h, partition, target, ptr, n, kind))

    def UpdateAsync(self, gradient, partition: int, from_clients: bool = True, *, big_endian: bool = True) -> int:
        """Updater._Update without waiting.  ``gradient`` is a PinnedBuffer (the
        `ipfs cat` bytes, big-endian unless ``big_endian=False``) that the fold
        reads over PCIe, or a DeviceBuffer that is queued and folded with the
        partition's other queued buckets in one launch (set_coalesce).  Returns
        a ticket; keep the buffer until Wait(ticket)."""
        target = N.TGT_AGG if from_clients else N.TGT_REP
        if self._fast is not None and isinstance(gradient, DeviceBuffer):
            t = self._fast.accumulate_async(self._hv, partition, target, gradient.ptr, gradient.n, gradient.kind)
            if t < 0:
                self._chk(t)
            return t
        t = ctypes.c_uint64()
        if isinstance(gradient, DeviceBuffer):
            rc = self._lib.ipls_agg_accumulate_async(self._h, partition, target, gradient.ptr, gradient.n,
                                                     gradient.kind, ctypes.byref(t))
            if rc < 0:
                self._chk(rc)
            return t.value
        if not isinstance(gradient, PinnedBuffer):
            raise TypeError("UpdateAsync takes a PinnedBuffer (ipls_host_alloc memory) or a DeviceBuffer")
        if self._fast is not None:
            t = self._fast.accumulate_async(self._hv, partition, target, gradient.ptr, gradient.nbytes // 8,
                                            N.HOST_BE if big_endian else N.HOST_F64)
            if t < 0:
                self._chk(t)
            return t
        self._chk(self._lib.ipls_agg_accumulate_async(self._h, partition, target, gradient.ptr,
                                                      gradient.nbytes // 8,
                                                      N.HOST_BE if big_endian else N.HOST_F64, ctypes.byref(t)))
        return t.value

    def UpdateAsyncMany(self, arrivals, from_clients: bool = True, *, big_endian: bool = True) -> int:
        """UpdateAsync for several arrivals in order, e.g. every bucket the
        Updater's queue holds at once (one peer's partitions): ``arrivals`` is
        a sequence of (gradient, partition) with DeviceBuffer or PinnedBuffer
        gradients.  Through ipls._fast it is one Python -> C transition for
        the whole list; the folds, their order and their bits are those of
        one UpdateAsync per arrival.  Returns the last ticket (0 for an empty
        list).  An error stops at the failing arrival: the earlier ones are
        queued, as after the same UpdateAsync calls."""
        target = N.TGT_AGG if from_clients else N.TGT_REP
        items = []
        for g, p in arrivals:
            if isinstance(g, DeviceBuffer):
                items.append((p, g.ptr, g.n, g.kind))
            elif isinstance(g, PinnedBuffer):
                items.append((p, g.ptr, g.nbytes // 8, N.HOST_BE if big_endian else N.HOST_F64))
            else:
                raise TypeError("UpdateAsyncMany takes DeviceBuffer or PinnedBuffer gradients")
        if not items:
            return 0
        if self._fast is not None:
            t = self._fast.accumulate_async_many(self._hv, target, items)
            if isinstance(t, tuple):
                self._chk(t[0])
            return t
        t = ctypes.c_uint64()
        for p, ptr, n, kind in items:
            self._chk(self._lib.ipls_agg_accumulate_async(self._h, p, target, ptr, n, kind, ctypes.byref(t)))
        return t.value

    def UpdateChunked(self, partition: int, n: int, source, *, big_endian: bool = True, from_clients: bool = True,
                      chunk: int = 1 << 19, dtype=None):
        """Updater._Update of one bucket that the caller produces chunk by
        chunk, as ONE library call (ipls_agg_accumulate_chunked): ``source(dst,
        offset, count)`` writes the bucket's values [offset, offset + count)
        -- 8*count bytes, big-endian unless ``big_endian=False`` -- at the
        address ``dst`` (the library's pinned ring) and returns True; False
        stops the call with nothing folded.  ``n`` is the bucket's length
        (shorter than the partition: ArrayIndexOutOfBounds, before any
        source call).  ``dtype=np.float32``, ``np.float16`` or ``"bf16"``: a
        trainer's bucket (ipls_agg_accumulate_chunked_narrow) -- the source
        writes 4*count or 2*count bytes of that format in native byte order
        (``big_endian`` does not apply), ``n``, ``chunk``, offset and count
        still in elements; the values are widened on the GPU."""
        kind = None if dtype is None else _HOST_KIND[_chunked_dtype(dtype)]
        target = N.TGT_AGG if from_clients else N.TGT_REP
        caught = []

        @N.CHUNK_SOURCE
        def cb(ctx, dst, off, cnt):
            return _callback(caught, source, dst, off, cnt)
        if kind is not None:
            rc = self._lib.ipls_agg_accumulate_chunked_narrow(self._h, partition, target, n, kind, chunk, cb, None)
        else:
            rc = self._lib.ipls_agg_accumulate_chunked(self._h, partition, target, n,
                                                       N.HOST_BE if big_endian else N.HOST_F64, chunk, cb, None)
        _reraise(caught)
        self._chk(rc)

    def UpdateGradientChunked(self, n: int, source, auth_list, *, big_endian: bool = True, dtype=None,
                              chunk: int = 1 << 19):
        """UpdateGradient (IPLS.java:1708-1743) of one whole flat gradient
        of ``n`` values that the caller produces chunk by chunk, as ONE library
        call (ipls_agg_update_gradient_chunked): the bits of UpdateGradient on
        the same vector, applied to every partition of ``auth_list`` at one
        instant once the last chunk has landed, or not at all.  ``source(dst,
        offset, count)`` writes the vector's values [offset, offset + count)
        at the address ``dst`` (the library's pinned ring) and returns True;
        False stops the call with every partition untouched.  It is called for
        consecutive chunks of the whole vector, also where no listed partition
        has values (a socket source must consume the stream).  ``dtype`` and
        ``big_endian`` as in UpdateChunked: 8*count big-endian bytes by
        default, native doubles with ``big_endian=False``, or 4*count / 2*count
        bytes of ``np.float32`` / ``np.float16`` / ``"bf16"``."""
        kind = (N.HOST_BE if big_endian else N.HOST_F64) if dtype is None else _HOST_KIND[_chunked_dtype(dtype)]
        owned = np.ascontiguousarray(np.asarray(list(auth_list), dtype=np.int32))
        caught = []

        @N.CHUNK_SOURCE
        def cb(ctx, dst, off, cnt):
            return _callback(caught, source, dst, off, cnt)
        rc = self._lib.ipls_agg_update_gradient_chunked(
            self._h, n, kind, owned.ctypes.data_as(ctypes.c_void_p), len(owned), chunk, cb, None)
        _reraise(caught)
        self._chk(rc)

    def GetPartitionsChunked(self, sink, *, wire: bool = False, chunk: int = 1 << 19, dtype=None):
        """GetPartitions (IPLS.java:1159-1174) handed to ``sink(ptr, offset,
        count)`` chunk by chunk in model order (ipls_agg_get_partitions_chunked,
        or with ``wire=True`` the Middleware task-3 writeDouble stream,
        ipls_agg_get_partitions_wire_chunked): 8*count bytes at ``ptr`` in
        the library's pinned ring, valid during the call; the sink returns
        True to go on.  ``dtype=np.float32``, ``np.float16`` or ``"bf16"``: the
        model narrowed on the GPU as GetPartitions(dtype=...) narrows it
        (ipls_agg_get_partitions_chunked_narrow); the call is then ``sink(ptr,
        byte_offset, byte_count)`` over the narrowed flat model, every piece a
        whole number of elements, ``chunk`` still in elements.  ``wire=True``
        holds doubles: together with a dtype it is a ValueError."""
        caught = []
        if dtype is not None:
            kind = _HOST_KIND[_chunked_dtype(dtype)]
            if wire:
                raise ValueError("wire=True is the big-endian double stream: it takes no dtype")

            @N.BYTE_SINK
            def bcb(ctx, b, off, cnt):
                return _callback(caught, sink, ctypes.cast(b, ctypes.c_void_p).value, off, cnt)
            rc = self._lib.ipls_agg_get_partitions_chunked_narrow(self._h, kind, chunk, bcb, None)
            _reraise(caught)
            self._chk(rc)
            return

        @N.CHUNK_SINK
        def cb(ctx, vals, off, cnt):
            return _callback(caught, sink, ctypes.cast(vals, ctypes.c_void_p).value, off, cnt)
        fn = self._lib.ipls_agg_get_partitions_wire_chunked if wire else self._lib.ipls_agg_get_partitions_chunked
        rc = fn(self._h, chunk, cb, None)
        _reraise(caught)
        self._chk(rc)

    def AggregatePartitionChunked(self, partition: int, sink, *, big_endian: bool = True, chunk: int = 1 << 19):
        """AggregatePartition with the committed sum handed to ``sink(ptr,
        offset, count)`` chunk by chunk, as one call (ipls_agg_finalize_chunked:
        no other caller's call lands between the sum and its bytes)."""
        caught = []

        @N.CHUNK_SINK
        def cb(ctx, vals, off, cnt):
            return _callback(caught, sink, ctypes.cast(vals, ctypes.c_void_p).value, off, cnt)
        rc = self._lib.ipls_agg_finalize_chunked(self._h, partition, N.HOST_BE if big_endian else N.HOST_F64,
                                                 chunk, cb, None)
        _reraise(caught)
        self._chk(rc)

    def flush(self):
        """Launch the folds of every queued device bucket now (no wait)."""
        self._chk(self._lib.ipls_agg_flush(self._h))

    def set_coalesce(self, max_group: int):
        """Largest group of queued device buckets folded per partition in one launch."""
        self._chk(self._lib.ipls_agg_set_coalesce(self._h, max_group))

    def Wait(self, ticket: int):
        """Block until the UpdateAsync fold ``ticket`` (and all before it) is done."""
        self._chk(self._lib.ipls_agg_wait(self._h, ticket))

    def UpdateIndirect(self, file_bytes, partition: int, from_clients: bool = True, *,
                       from_future: bool = False):
        """Updater.run for a queue item with only a hash (Updater.java:176-187):
        GetParameters(hash, Gradient_Buff) then _Update(Gradient_Buff, ...),
        with the reference's reusable Gradient_Buff (a short file folds the
        previous request's tail; a file longer than the buffer raises the
        AIOOBE after overwriting it).  ``file_bytes``: the `ipfs cat` bytes."""
        target = N.TGT_FUTURE if from_future else (N.TGT_AGG if from_clients else N.TGT_REP)
        if isinstance(file_bytes, PinnedBuffer):
            ptr, nb = file_bytes.ptr, file_bytes.nbytes
        else:
            a = np.frombuffer(bytes(file_bytes), dtype=np.uint8)
            ptr, nb = (a.ctypes.data if a.size else None), a.size
        self._chk(self._lib.ipls_agg_update_indirect(self._h, partition, target, ptr, nb))

    def PromoteFuture(self, partitions):
        """End of Update_Client_WaitAck_List (IPLS.java:1556-1562): for p in
        ``partitions`` (the Auth_List), Aggregated_Gradients[p] =
        Aggregated_Gradients_from_future[p], and the latter is zeroed."""
        parts = np.ascontiguousarray(list(partitions), dtype=np.int32)
        self._chk(self._lib.ipls_agg_promote_future(
            self._h, parts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), parts.size))

    def ingest_pubsub(self, messages, *, from_clients: bool = True, layers: int = 2, partitions=None):
        """ThreadReceiver (IPLS.java:851-866, 453-465): a batch of pubsub
        'data' texts -> base64url x layers -> GET_GRADIENTS frame -> fold, all
        on the GPU.  Returns (number folded, per-message status)."""
        msgs = [np.frombuffer(bytes(m), dtype=np.uint8) for m in messages]
        n = len(msgs)
        ptrs = (ctypes.c_void_p * max(1, n))(*[m.ctypes.data if m.size else None for m in msgs])
        lens = (ctypes.c_int64 * max(1, n))(*[m.size for m in msgs])
        st = (ctypes.c_int32 * max(1, n))()
        parts = None
        if partitions is not None:
            parts = (ctypes.c_int32 * max(1, n))(*partitions)
        target = N.TGT_AGG if from_clients else N.TGT_REP
        k = self._chk(self._lib.ipls_agg_ingest_pubsub(self._h, target, ptrs, lens, n, layers, parts, st))
        return k, list(st)[:n]

    # ---- -async true variants (Updater.java:57-69, 197-199) ----
    ASYNC_DECAY = 0.75      # Updater.java:58
    LEAVING_A = 0.6         # Updater.java:17 (field a)

    def UpdateAsyncReplica(self, gradient, partition: int):
        """Async replica fold: W = 0.75*W + g (Updater.java:57-59)."""
        ptr, n, kind, keep = _operand(gradient)
        self._chk(self._lib.ipls_agg_blend(self._h, partition, N.TGT_WEIGHTS, ptr, n, kind, 0.75, 1.0))

    def UpdateLeavingPeer(self, weights, partition: int):
        """Leaving peer's weights: W = a*W + (1-a)*w, a = 0.6 (Updater.java:65-69)."""
        a = self.LEAVING_A
        ptr, n, kind, keep = _operand(weights)
        self._chk(self._lib.ipls_agg_blend(self._h, partition, N.TGT_WEIGHTS, ptr, n, kind, a, 1 - a))

    def AsyncPublishScale(self, partition: int):
        """Aggregated = 0.25*Weights before the async publish (Updater.java:197-199)."""
        self._chk(self._lib.ipls_agg_scale(self._h, partition, N.TGT_AGG, N.TGT_WEIGHTS, 0.25))

    def OtherReplicaGradients(self, partition: int, aggregator: int, gradients, *, key_hash: int | None = None):
        """Download_Scheduler.download_gradients (Download_Scheduler.java:245-268):
        a bucket that another aggregator of ``partition`` will also fold.  The
        first one becomes Other_Replica_Gradients[(p, a)], later ones fold into
        it.  ``aggregator`` is the int the caller maps 1:1 from the aggregator's
        peer-ID String; ``key_hash`` is ``new Pair<>(p, peerId).hashCode()``
        (java_pair_hash), which places the key in the HashMap and so fixes the
        Collect_Replicas order.  Without it the peer ID is str(aggregator)."""
        ptr, n, kind, keep = _operand(gradients)
        if key_hash is None:
            self._chk(self._lib.ipls_agg_other_replica(self._h, partition, aggregator, ptr, n, kind))
        else:
            self._chk(self._lib.ipls_agg_other_replica_keyed(self._h, partition, aggregator,
                                                             ctypes.c_int32(key_hash).value, ptr, n, kind))

    def OtherReplicaDrop(self, partition: int, aggregator: int) -> bool:
        """Other_Replica_Gradients.remove(new Pair<>(p, a)) with its received
        count (Download_Scheduler.java:215-217, 329-332, 438-440): that
        aggregator's own partial arrived, so its downloaded buckets are not
        collected.  True if the key was stored."""
        return self._chk(self._lib.ipls_agg_other_replica_drop(self._h, partition, aggregator)) == 1

    def replica_order(self):
        """(keys, capacity): the (partition, aggregator) order Collect_Replicas
        would fold in now -- the library's model of the JDK HashMap's keySet()
        order -- and the model's table capacity."""
        room = self._chk(self._lib.ipls_agg_replica_order(self._h, None, 0, None))
        cap = ctypes.c_int32()
        while True:   # keys stored by another thread in between: ask again with more room
            buf = (ctypes.c_int32 * max(2, 2 * room))()
            n = self._chk(self._lib.ipls_agg_replica_order(self._h, buf, room, ctypes.byref(cap)))
            if n <= room:
                return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)], cap.value
            room = n

    def Collect_Replicas(self):
        """IPLS.java:1217-1241: fold every stored Other_Replica_Gradients array
        into REP in the JDK HashMap's key-set order and clear the store.
        Returns (arrays folded, per-partition Participants increments: each
        stored key adds received x its length, IPLS.java:1229-1234 updating
        Participants inside the element loop)."""
        part = (ctypes.c_int32 * max(1, self.n_partitions))()
        k = self._chk(self._lib.ipls_agg_collect_replicas(self._h, part))
        return k, list(part)[:self.n_partitions]

    def reduce_batch(self, p_first: int, buckets, *, start_mode: int = N.START_ZERO,
                     target: int = N.TGT_AGG, big_endian: bool = False):
        """One launch over len(buckets) partitions; buckets[q] is the list of
        device pointers (ints or DeviceBuffers) for partition p_first+q."""
        n_parts = len(buckets)
        flat, k, kind = _bucket_table_kind(buckets, self.lengths, p_first, big_endian)
        arr = (ctypes.c_void_p * max(1, len(flat)))(*flat)
        self._chk(self._lib.ipls_agg_reduce_batch(self._h, p_first, n_parts, arr, k, kind,
                                                  start_mode, target))

    def reduce_batch_out(self, p_first: int, buckets, dsts, *, start_mode: int = N.START_ZERO,
                         big_endian_in: bool = False, big_endian_out: bool = False):
        """Batched fold into caller device buffers ``dsts[q]`` (one per
        partition); ``big_endian_out`` fuses the update_file byte pack."""
        n_parts = len(buckets)
        if len(dsts) != n_parts:
            raise ValueError("need k buckets and one destination per partition")
        flat, k, kind = _bucket_table_kind(buckets, self.lengths, p_first, big_endian_in)
        for q, d in enumerate(dsts):
            p = p_first + q
            if isinstance(d, DeviceBuffer) and d.dtype != "f64":
                raise N.IplsError(N.IPLS_E_INVAL, f"reduce_batch_out writes doubles or big-endian bytes, not {d.dtype}")
            if isinstance(d, DeviceBuffer) and 0 <= p < self.n_partitions and d.n < self.lengths[p]:
                raise ValueError(f"partition {p} needs a destination of {self.lengths[p]} doubles, "
                                 f"the DeviceBuffer holds {d.n}")
        arr = (ctypes.c_void_p * max(1, len(flat)))(*flat)
        darr = (ctypes.c_void_p * max(1, n_parts))(*[d.ptr if isinstance(d, DeviceBuffer) else int(d) for d in dsts])
        self._chk(self._lib.ipls_agg_reduce_batch_out(
            self._h, p_first, n_parts, arr, k, kind, start_mode,
            darr, N.DEV_BE if big_endian_out else N.DEV_F64))

    def aggregate_round(self, p_first: int, buckets, *, big_endian: bool = False, with_average: bool = True,
                        out=None, dtype=np.float64):
        """A whole round in one launch: the folds of ``buckets`` (buckets[q] =
        device buckets of partition p_first+q, may be empty lists) into AGG,
        AggregatePartition (IPLS.java:1248-1274) and the GetPartitions divide
        (IPLS.java:1159-1174).  Returns the averaged values of the partitions
        (host array, or ``out`` when a DeviceBuffer is given), or None.
        f32, half and bf16 buckets are widened in the fold; an f32 ``out`` (or
        ``dtype=np.float32`` for the host array) gets the averages narrowed
        once to float, as Model.java:388-390 narrows them; a half / bf16
        ``out`` (or ``dtype=np.float16`` / ``dtype="bf16"``, the latter a
        uint16 array of bit patterns) gets that float rounded again to the
        16-bit format (include/ipls_agg.h: two roundings, what narrowing the
        f32 output gives).
        One launch means: f64 buckets with f64 averages (k_round), and f32 /
        half / bf16 buckets with no averages or f32 / half / bf16 ones
        (k_round_narrow; ``with_average=False``, an ``out`` of one of these
        dtypes, or such a ``dtype=``), every bucket 16-B aligned.  Everything
        else -- a bucket off a 16-B boundary, f32 / half / bf16 buckets with
        the default f64 averages, f64 buckets with narrowed averages -- runs
        the fold, AggregatePartition and the divide as three launches inside
        the call, with the same bits."""
        n_parts = len(buckets)
        flat, k, kind = _bucket_table_kind(buckets, self.lengths, p_first, big_endian)
        arr = (ctypes.c_void_p * max(1, len(flat)))(*flat)
        ap, ak, res = None, N.HOST_F64, None
        if isinstance(out, DeviceBuffer):
            if n_parts and 0 <= p_first and p_first + n_parts <= self.n_partitions:
                last = p_first + n_parts - 1
                need = self.offsets[last] + self.lengths[last] - 1 - self.offsets[p_first]
                if out.n < need:
                    raise ValueError(f"the averages of partitions {p_first}..{last} need {need} values, "
                                     f"the DeviceBuffer holds {out.n}")
            ap, ak, res = out.ptr, _DEV_KIND.get(out.dtype, N.DEV_F64), out
        elif with_average:
            last = p_first + n_parts - 1
            n = self.offsets[last] + self.lengths[last] - 1 - self.offsets[p_first]
            od = _out_dtype(dtype)
            res = np.empty(max(0, n), dtype=_NP_OUT[od])
            ak = _HOST_KIND.get(od, N.HOST_F64)
            ap = res.ctypes.data if res.size else None
        self._chk(self._lib.ipls_agg_aggregate_round(self._h, p_first, n_parts, arr, k, kind, ap, ak))
        return res

    def commit_partial_update(self, partition: int, workers: int) -> bytes:
        """IPLS_Comm.commit_partial_update (IPLS_Comm.java:51-61, called at
        IPLS.java:1423-1425): the Java-serialised new Pair<>(workers,
        Aggregated_Gradients[p]) file bytes, packed on the device."""
        n = self._chk(self._lib.ipls_agg_commit_partial(self._h, partition, workers, None, 0))
        out = np.empty(n, dtype=np.uint8)
        self._chk(self._lib.ipls_agg_commit_partial(self._h, partition, workers, out.ctypes.data, n))
        return out.tobytes()

    # ---- saved-model files (IPLS.save_model / DownloadMapParameters) ----
    def _two_calls(self, fn, *args) -> bytes:
        """A size-then-fill entry point: fn(handle, *args, out, out_cap)."""
        n = self._chk(fn(self._h, *args, None, 0))
        out = np.empty(n, dtype=np.uint8)
        self._chk(fn(self._h, *args, out.ctypes.data, n))
        return out.tobytes()

    def save_model(self, auth_list=None, *, sink=None, target: int = N.TGT_WEIGHTS, chunk_bytes: int = 4 << 20):
        """IPLS.save_model (IPLS.java:1904-1911): the Java-serialised
        HashMap<Integer,double[]> of Weights[p] for p in ``auth_list`` (default:
        every partition), packed on the device.  Returns the file's bytes, or
        with ``sink(ptr, offset, count)`` hands them over piece by piece
        (ipls_agg_save_model_chunked; the sink returns True to go on)."""
        parts = list(range(self.n_partitions)) if auth_list is None else [int(p) for p in auth_list]
        cp = (ctypes.c_int32 * max(len(parts), 1))(*parts)
        if sink is None:
            return self._two_calls(self._lib.ipls_agg_save_model, cp, len(parts), target)
        caught = []

        @N.BYTE_SINK
        def cb(ctx, b, off, cnt):
            return _callback(caught, sink, ctypes.cast(b, ctypes.c_void_p).value, off, cnt)
        rc = self._lib.ipls_agg_save_model_chunked(self._h, cp, len(parts), target, chunk_bytes, cb, None)
        _reraise(caught)
        self._chk(rc)
        return None

    def save_partition(self, partition: int, *, target: int = N.TGT_WEIGHTS) -> bytes:
        """The serialised double[] of one partition: the single-partition
        hand-over file (MyIPFSClass.java:261-270, IPLS.java:136-140)."""
        return self._two_calls(self._lib.ipls_agg_save_partition, partition, target)

    def save_model_list(self, *, target: int = N.TGT_WEIGHTS) -> bytes:
        """The serialised ArrayList<Double> of every partition's values in
        order: the pid-5 `<ID>Model` reply and init's `<ID>ETHModel`
        (IPLS.java:547-558, 2255-2273)."""
        return self._two_calls(self._lib.ipls_agg_save_model_list, target)

    def LoadSavedModel(self, file_bytes, parts=None, *, leaving_peer: bool = False,
                       target: int = N.TGT_WEIGHTS) -> int:
        """DownloadMapParameters (MyIPFSClass.java:559-566) and what follows it:
        Weights[p] = file[p] for p in ``parts`` (the ChangedList; default every
        key of the file), or with ``leaving_peer=True`` the Updater's blend
        W = a*W + (1-a)*file[p], a = 0.6 (IPLS.java:728-731, Updater.java:65-69).
        Returns the number of partitions written."""
        a = _u8(file_bytes)
        cp, n = None, 0
        if parts is not None:
            parts = [int(p) for p in parts]
            cp, n = (ctypes.c_int32 * max(len(parts), 1))(*parts), len(parts)
        done = ctypes.c_int32()
        la = self.LEAVING_A
        self._chk(self._lib.ipls_agg_load_saved(self._h, a.ctypes.data, a.size,
                                                N.SAVED_BLEND if leaving_peer else N.SAVED_SET, target, cp, n,
                                                la, 1 - la, ctypes.byref(done)))
        return done.value

    def merge_files(self, files, *, partial_updates: bool = False) -> bytes:
        """Storage node merge (Decentralized_Storage_Receiver.java:239-258) of
        downloaded files -- raw BE gradient files (status 0) or Pair partial
        updates (status != 0) -- into the `_partial_aggregation` file bytes."""
        arrs = [np.frombuffer(bytes(f), dtype=np.uint8) for f in files]
        k = len(arrs)
        ptrs = (ctypes.c_void_p * max(1, k))(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (ctypes.c_int64 * max(1, k))(*[a.size for a in arrs])
        kind = N.HOST_PAIR if partial_updates else N.HOST_BE
        if k == 0:
            raise ValueError("need at least one file")
        if partial_updates:
            n0, _, _ = pair_parse(arrs[0])
            cap = 8 * len(n0)
        else:
            cap = 8 * (arrs[0].size // 8)
        out = np.empty(max(1, cap), dtype=np.uint8)
        nb = self._chk(self._lib.ipls_agg_merge_files(self._h, ptrs, lens, k, kind, out.ctypes.data, cap))
        return out[:nb].tobytes()

    def Merge(self, partition: int, buckets, *, big_endian: bool = True, target: int = N.TGT_REP):
        """Storage-node merge (Decentralized_Storage_Receiver.java:239-247):
        S = g0; S += g_i -- a FIRST-start fold (it overwrites ``target``, so call
        it on the storage node's own Aggregator), returned as BE file bytes
        (the ``<p>_partial_aggregation`` file, :258)."""
        self.reduce_batch(partition, [list(buckets)], start_mode=N.START_FIRST, target=target,
                          big_endian=big_endian)
        return self.read(partition, target, big_endian=True)

    def AggregatePartition(self, partition: int, *, with_sum: bool = False, sum_big_endian: bool = True,
                           with_average: bool = False, sum_out=None):
        """IPLS.java:1248-1274.  Optionally returns the committed sum (the
        update_file bytes of IPLS_Comm.commit_update) and the averaged values.
        ``sum_out`` (a PinnedBuffer of at least 8*L_p bytes) receives the sum
        instead of a new pageable array: the D2H then runs at the PCIe rate."""
        L = self.lengths[partition] if partition >= 0 else 0
        s = a = None
        sp, sk = None, N.HOST_F64
        if sum_out is not None:
            if not isinstance(sum_out, PinnedBuffer) or sum_out.nbytes < 8 * L:
                raise ValueError("sum_out must be a PinnedBuffer of at least 8*L_p bytes")
            s = sum_out.view(np.uint8 if sum_big_endian else np.float64)[:8 * L if sum_big_endian else L]
            sp, sk = sum_out.ptr, (N.HOST_BE if sum_big_endian else N.HOST_F64)
        elif with_sum:
            s = np.empty(8 * L, dtype=np.uint8) if sum_big_endian else np.empty(L)
            sp, sk = s.ctypes.data, (N.HOST_BE if sum_big_endian else N.HOST_F64)
        ap = None
        if with_average:
            a = np.empty(max(0, L - 1))
            ap = a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self._chk(self._lib.ipls_agg_finalize(self._h, partition, sp, sk, ap))
        return s, a

    def cache_partition(self, partition: int, data, *, frame: bool = False):
        """Download_Scheduler.cache_partition: Weight_Address[p] = GetParameters(hash).
        ``frame=True``: the pid-4 ACK frame of ThreadReceiver (IPLS.java:491-498)."""
        if frame:
            a = np.frombuffer(bytes(data), dtype=np.uint8)
            self._chk(self._lib.ipls_agg_set_weights(self._h, partition, a.ctypes.data, a.size, N.HOST_FRAME))
            return
        ptr, n, kind, keep = _operand(data)
        self._chk(self._lib.ipls_agg_set_weights(self._h, partition, ptr, n, kind))

    def GetPartitions(self, *, wire: bool = False, out=None, dtype=np.float64):
        """IPLS.java:1140-1174: the averaged flat model.  ``wire=True`` returns
        the Middleware task-3 byte stream (DataOutputStream.writeDouble);
        with ``out`` a PinnedBuffer it is written there (the D2H at the PCIe
        rate) and a memoryview of those 8*M bytes is returned, ready for
        ``sendall`` without another copy.  An f32 DeviceBuffer ``out``, or
        ``dtype=np.float32`` for the host array, gets every value rounded once
        to float on the device (Model.java:388-390), 4 bytes per value.  A
        half / bf16 DeviceBuffer, ``dtype=np.float16`` (a numpy float16 array)
        or ``dtype="bf16"`` (a numpy uint16 array of the bfloat16 bit
        patterns) gets that float rounded again to the 16-bit format, 2 bytes
        per value.  A ``Segments`` ``out`` (the model's parameter tensors)
        gets every tensor written in its own dtype by those same rules, with
        no flat model and no copy-out in between; a ``ModelCopies`` ``out``
        (K trainers' tensors and the received model) gets every one of its
        lists written so, by one call."""
        n = self.flat_size
        if isinstance(out, Difference):
            raise TypeError("a Difference is an operand of UpdateGradient and SendGradients only, not an output")
        if isinstance(out, PeerUpdates):
            raise TypeError("a PeerUpdates is an operand of UpdateGradient only, not an output")
        if isinstance(out, ModelCopies):   # every list of one architecture in one launch (k_divide_segs_copies)
            self._chk(self._lib.ipls_agg_get_partitions_segs_copies(self._h, *out.tables))
            return out
        if isinstance(out, Segments):   # straight into the model's tensors, each in its own dtype (k_divide_segs)
            self._chk(self._lib.ipls_agg_get_partitions_segs(self._h, *out.tables))
            return out
        if isinstance(out, DeviceBuffer):
            self._chk(self._lib.ipls_agg_get_partitions(self._h, out.ptr, out.n, _DEV_KIND.get(out.dtype, N.DEV_F64)))
            return out
        od = _out_dtype(dtype)
        if od != "f64" and out is None and not wire:
            buf = np.empty(n, dtype=_NP_OUT[od])
            self._chk(self._lib.ipls_agg_get_partitions(self._h, buf.ctypes.data, n, _HOST_KIND[od]))
            return buf
        if isinstance(out, PinnedBuffer):
            if out.nbytes < 8 * n:
                raise ValueError(f"PinnedBuffer of {out.nbytes} bytes < the model's {8 * n}")
            kind = N.HOST_BE_CANON if wire else N.HOST_F64
            self._chk(self._lib.ipls_agg_get_partitions(self._h, out.ptr, n, kind))
            v = out.view()[:8 * n]
            return memoryview(v) if wire else v.view(np.float64)
        if wire:
            buf = np.empty(8 * n, dtype=np.uint8)
            self._chk(self._lib.ipls_agg_get_partitions(self._h, buf.ctypes.data, n, N.HOST_BE_CANON))
            return buf.tobytes()
        buf = np.empty(n)
        self._chk(self._lib.ipls_agg_get_partitions(self._h, buf.ctypes.data, n, N.HOST_F64))
        return buf

    # ---- replica exchange hooks (ipls.distributed) ----
    def export_partial(self, partition: int, tensor):
        """Copy this aggregator's partial sum AGG[p] into a transport tensor
        (the published partial of IPLS.java:1423-1431) and wait for it.  A
        device tensor (RCCL) gets a device-to-device copy, a host tensor
        (gloo) a device-to-host copy."""
        if getattr(tensor, "is_cuda", False):
            d = DeviceBuffer.from_tensor(tensor)
            self._chk(self._lib.ipls_agg_read(self._h, partition, N.TGT_AGG, d.ptr, d.n, N.DEV_F64))
            self.sync()
        else:
            self._chk(self._lib.ipls_agg_read(self._h, partition, N.TGT_AGG, int(tensor.data_ptr()),
                                              tensor.numel(), N.HOST_F64))

    def import_partial(self, partition: int, tensor, *, replace_agg: bool = False):
        """Fold a replica's partial (a transport tensor that has landed) into
        REP[p] (Updater.java:40-44); replace_agg stores it as AGG[p] instead."""
        if not getattr(tensor, "is_cuda", False):
            if not replace_agg:
                self.Update(tensor.numpy(), partition, from_clients=False)
                return
            # exact FIRST-start copy needs a device operand: on the GPU of the
            # shard that owns the partition (the one whose kernel reads it)
            tensor = tensor.to(f"cuda:{self.partition_device(partition)[0]}")
        d = DeviceBuffer.from_tensor(tensor)
        if replace_agg:
            self.reduce_batch(partition, [[d]], start_mode=N.START_FIRST, target=N.TGT_AGG)
        else:
            self.Update(d, partition, from_clients=False)

    # ---- multi-GPU: shards and replica slots (include/ipls_agg.h, cfg.devices) ----
    def partition_device(self, partition: int):
        """(device ordinal, HIP stream) of the shard that owns ``partition``."""
        d, st = ctypes.c_int32(), ctypes.c_void_p()
        self._chk(self._lib.ipls_agg_partition_device(self._h, partition, ctypes.byref(d), ctypes.byref(st)))
        return d.value, int(st.value or 0)

    def reduce_partial(self, slot: int, p_first: int, buckets, *, start_mode: int = N.START_ZERO,
                       big_endian: bool = False):
        """Replica slot ``slot`` (a shard that does not own these partitions)
        folds buckets resident on its GPU into its partial sums (an aggregator
        of the partition other than its owner, IPLS.java:1402-1431)."""
        n_parts = len(buckets)
        flat, k, bk = _bucket_table_kind(buckets, self.lengths, p_first)
        if bk not in (N.DEV_F64, N.DEV_BE):
            raise N.IplsError(N.IPLS_E_INVAL, "reduce_partial takes f64 buckets (DEV_F64/DEV_BE)")
        arr = (ctypes.c_void_p * max(1, len(flat)))(*flat)
        self._chk(self._lib.ipls_agg_reduce_partial(self._h, slot, p_first, n_parts, arr, k,
                                                    N.DEV_BE if big_endian else N.DEV_F64, start_mode))

    def combine_partials(self, p_first: int = 0, n_parts: int | None = None) -> int:
        """REP[p] += every slot's partial of p, slots ascending, read over xGMI
        by the owner's fold kernel (Collect_Replicas, IPLS.java:1449).
        Returns the number of partials folded."""
        n = self.n_partitions - p_first if n_parts is None else n_parts
        return self._chk(self._lib.ipls_agg_combine_partials(self._h, p_first, n))

    # ---- publish-side codec (a9) ----
    @staticmethod
    def _device_text_out(out, out_cap, need: int):
        """(address, capacity in bytes) of a device text destination.  A
        DeviceBuffer's capacity is its own size (8 * n); a raw address must come
        with ``out_cap`` -- the library can only bound its writes by what it is
        told, so an undersized buffer is refused here, never written past."""
        if isinstance(out, DeviceBuffer):
            ptr, cap = out.ptr, 8 * out.n
            if out_cap is not None:
                cap = min(cap, int(out_cap))
        else:
            if out_cap is None:
                raise ValueError("a raw device address needs out_cap= (its capacity in bytes)")
            ptr, cap = int(out), int(out_cap)
        if cap < need:
            raise ValueError(f"publish text needs {need} bytes, the device buffer holds {cap}")
        return ptr, cap

    def publish_partial(self, partition: int, a: int, b: int, *, pid: int = 3, origin: bytes = b"",
                        target: int = N.TGT_AGG, out=None, out_cap: int | None = None) -> bytes | int:
        """Marshall_Packet(target[p], origin, a, b, pid) as Base64.getUrlEncoder
        text (MyIPFSClass.java:990-1016; IPLS.java:1429-1430 publishes AGG with
        a = iteration, b = workers + 1, pid 3), encoded on the GPU.  Returns the
        text bytes, or its length when ``out`` is a DeviceBuffer / int address
        with ``out_cap`` bytes (device text, stream-ordered) or a PinnedBuffer
        (host text)."""
        o = np.frombuffer(bytes(origin), dtype=np.uint8)
        op = o.ctypes.data if o.size else None
        n = self._chk(self._lib.ipls_agg_publish_partial(self._h, partition, target, a, b, pid, op, o.size,
                                                         None, 0, N.HOST_TEXT))
        if isinstance(out, PinnedBuffer):   # host text into pinned memory: the D2H runs at the PCIe rate
            if out.nbytes < n:
                raise ValueError(f"publish text needs {n} bytes")
            return self._chk(self._lib.ipls_agg_publish_partial(self._h, partition, target, a, b, pid, op,
                                                                o.size, out.ptr, n, N.HOST_TEXT))
        if out is not None:
            ptr, cap = self._device_text_out(out, out_cap, n)
            return self._chk(self._lib.ipls_agg_publish_partial(self._h, partition, target, a, b, pid, op,
                                                                o.size, ptr, cap, N.DEV_TEXT))
        buf = np.empty(max(1, n), dtype=np.uint8)
        self._chk(self._lib.ipls_agg_publish_partial(self._h, partition, target, a, b, pid, op, o.size,
                                                     buf.ctypes.data, n, N.HOST_TEXT))
        return buf[:n].tobytes()

    def publish_partials(self, partitions, a: int, b, *, pid: int = 3, origin: bytes = b"",
                         target: int = N.TGT_AGG, out=None, out_cap: int | None = None):
        """The publish loop over Auth_List (IPLS.java:1423-1431) in one launch
        per GPU: text i = Marshall_Packet(target[partitions[i]], origin, a,
        b[i], pid) base64url-encoded.  Returns the list of texts (bytes), or,
        when ``out`` is a DeviceBuffer / device address with ``out_cap`` bytes /
        PinnedBuffer, the (lens, offs) of the texts written there (device:
        stream-ordered)."""
        parts = np.ascontiguousarray(list(partitions), dtype=np.int32)
        bb = np.ascontiguousarray(list(b), dtype=np.int32)
        if bb.size != parts.size:
            raise ValueError("one b value per partition")
        o = np.frombuffer(bytes(origin), dtype=np.uint8)
        op = o.ctypes.data if o.size else None
        n = parts.size
        lens = np.zeros(max(1, n), dtype=np.int64)
        offs = np.zeros(max(1, n), dtype=np.int64)
        total = self._chk(self._lib.ipls_agg_publish_partials(
            self._h, parts.ctypes.data, n, target, a, bb.ctypes.data, pid, op, o.size, None, 0, N.HOST_TEXT,
            lens.ctypes.data, offs.ctypes.data))
        if out is not None:
            if isinstance(out, PinnedBuffer):
                ptr, cap, kind = out.ptr, out.nbytes, N.HOST_TEXT
            else:
                (ptr, cap), kind = self._device_text_out(out, out_cap, total), N.DEV_TEXT
            self._chk(self._lib.ipls_agg_publish_partials(
                self._h, parts.ctypes.data, n, target, a, bb.ctypes.data, pid, op, o.size, ptr, cap, kind,
                None, None))
            return lens[:n].tolist(), offs[:n].tolist()
        buf = np.empty(max(1, total), dtype=np.uint8)
        self._chk(self._lib.ipls_agg_publish_partials(
            self._h, parts.ctypes.data, n, target, a, bb.ctypes.data, pid, op, o.size, buf.ctypes.data, total,
            N.HOST_TEXT, None, None))
        return [buf[offs[i]:offs[i] + lens[i]].tobytes() for i in range(n)]

    def SendGradients(self, gradients, partitions, iteration: int, *, origin: bytes = b"", pid: int = 3, out=None,
                      out_cap: int | None = None):
        """SendGradients -> Send_Gradient_Partition (IPLS.java:1350-1400,
        1290-1322, direct mode): text i = Base64.getUrlEncoder(Marshall_Packet(
        OrganizeGradients(gradients)[partitions[i]], origin, partitions[i],
        iteration, pid)), encoded on the GPU straight from the flat vector in
        one launch per GPU.  ``gradients`` is what UpdateGradient takes (numpy
        float64 / float32 / float16, a CPU torch tensor, a DeviceBuffer), or
        ``None`` for the "did not train in time" texts (n = 0), or a
        ``Segments`` / list / tuple of CUDA tensors, encoded straight from the
        tensors.  A -0.0 stays
        -0.0 and the count slot is generated; the text is one base64 layer
        (the pubsub transport adds the second); secure mode's Encode is the
        caller's.  Returns the list of texts (bytes), or, when ``out`` is a
        DeviceBuffer / device address with ``out_cap`` bytes / PinnedBuffer,
        the (lens, offs) of the texts written there (device: stream-ordered)."""
        parts = np.ascontiguousarray(list(partitions), dtype=np.int32)
        o = np.frombuffer(bytes(origin), dtype=np.uint8)
        op = o.ctypes.data if o.size else None
        diff = gradients if isinstance(gradients, Difference) else None
        segs = None if diff is not None else _segments(gradients)
        if diff is not None or segs is not None or gradients is None:
            ptr, ng, kind, keep = None, 0, N.HOST_F64, None
        else:
            if getattr(gradients, "is_cuda", False):   # a GPU torch tensor: read where it lies
                gradients = DeviceBuffer.from_tensor(gradients)
            ptr, ng, kind, keep = _operand(gradients, f32=True)
        n = parts.size
        lens = np.zeros(max(1, n), dtype=np.int64)
        offs = np.zeros(max(1, n), dtype=np.int64)

        def call(dst, cap, dst_kind, le=None, of=None):
            if diff is not None:   # minuend - subtrahend, both read where they lie (k_b64url_encode_segs_diff)
                return self._chk(self._lib.ipls_agg_send_gradients_segs_diff(
                    self._h, *diff.tables, parts.ctypes.data, n, iteration, pid, op, o.size, dst, cap, dst_kind, le, of))
            if segs is not None:   # a list of device tensors, read where they lie (k_b64url_encode_segs)
                return self._chk(self._lib.ipls_agg_send_gradients_segs(
                    self._h, *segs.tables, parts.ctypes.data, n, iteration, pid, op, o.size, dst, cap, dst_kind, le, of))
            return self._chk(self._lib.ipls_agg_send_gradients(
                self._h, ptr, ng, kind, parts.ctypes.data, n, iteration, pid, op, o.size, dst, cap, dst_kind, le, of))

        total = call(None, 0, N.HOST_TEXT, lens.ctypes.data, offs.ctypes.data)
        if out is not None:
            if isinstance(out, PinnedBuffer):
                dst, cap, dst_kind = out.ptr, out.nbytes, N.HOST_TEXT
            else:
                (dst, cap), dst_kind = self._device_text_out(out, out_cap, total), N.DEV_TEXT
            call(dst, cap, dst_kind)
            return lens[:n].tolist(), offs[:n].tolist()
        buf = np.empty(max(1, total), dtype=np.uint8)
        call(buf.ctypes.data, total, N.HOST_TEXT)
        return [buf[offs[i]:offs[i] + lens[i]].tobytes() for i in range(n)]

    def last_launch(self) -> dict:
        """What the last fold launch ran (kernel, shape, lanes, vectors, SEQ code, map, grid)."""
        li = N.LaunchInfo()
        self._chk(self._lib.ipls_agg_last_launch(self._h, ctypes.byref(li)))
        return {f: getattr(li, f) for f, _ in N.LaunchInfo._fields_}

    # ---- state access ----
    def read(self, partition: int, target: int = N.TGT_AGG, *, big_endian: bool = False):
        L = self.lengths[partition]
        if big_endian:
            buf = np.empty(8 * L, dtype=np.uint8)
            self._chk(self._lib.ipls_agg_read(self._h, partition, target, buf.ctypes.data, L, N.HOST_BE))
            return buf.tobytes()
        buf = np.empty(L)
        self._chk(self._lib.ipls_agg_read(self._h, partition, target, buf.ctypes.data, L, N.HOST_F64))
        return buf

    def reset(self, partition: int = N.ALL_PARTITIONS):
        self._chk(self._lib.ipls_agg_reset(self._h, partition))

    def device_ptr(self, partition: int, target: int = N.TGT_AGG) -> int:
        p = ctypes.c_void_p()
        self._chk(self._lib.ipls_agg_device_ptr(self._h, partition, target, ctypes.byref(p)))
        return int(p.value)

    def checksum(self, partition: int, target: int = N.TGT_AGG) -> int:
        v = ctypes.c_uint64()
        self._chk(self._lib.ipls_agg_checksum(self._h, partition, target, ctypes.byref(v)))
        return int(v.value)


class PinnedBuffer:
    """Pinned host memory from ipls_host_alloc (what the Java side would wrap
    as a direct ByteBuffer).  Host operands in it are DMA'd without staging."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        N.check(N.lib().ipls_host_alloc(nbytes, ctypes.byref(p)))
        self.ptr = int(p.value or 0)
        self.nbytes = nbytes

    def view(self, dtype=np.uint8) -> np.ndarray:
        buf = (ctypes.c_char * self.nbytes).from_address(self.ptr)
        return np.frombuffer(buf, dtype=np.uint8).view(dtype)

    def close(self):
        if self.ptr:
            N.lib().ipls_host_free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- handle-free device utilities ----
def shard_plan(n_partitions: int, n_shards: int) -> list[int]:
    """Owner shard of every partition (contiguous blocks, p / ceil(P/G))."""
    out = (ctypes.c_int32 * max(1, n_partitions))()
    N.check(N.lib().ipls_shard_plan(n_partitions, n_shards, out))
    return list(out)[:n_partitions]


def java_pair_hash(p: int, peer_id: str) -> int:
    """new org.javatuples.Pair<Integer,String>(p, peer_id).hashCode() (the key
    hash of Other_Replica_Gradients, PeerData.java:140), computed by the
    library from the ID's UTF-8 bytes."""
    b = peer_id.encode("utf-8")
    buf = (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0")
    out = ctypes.c_int32()
    N.check(N.lib().ipls_java_pair_hash(p, ctypes.addressof(buf), len(b), ctypes.byref(out)))
    return out.value


def synth_fill(buf: DeviceBuffer, p: int, k: int, seed: int, stream: int = 0):
    N.check(N.lib().ipls_synth_fill(buf.ptr, buf.n, seed, p, k, buf.kind, stream or None))


def checksum_dev(buf: DeviceBuffer, n: int | None = None, stream: int = 0) -> int:
    v = ctypes.c_uint64()
    N.check(N.lib().ipls_checksum_dev(buf.ptr, buf.n if n is None else n, buf.kind,
                                      ctypes.byref(v), stream or None))
    return int(v.value)


def encode_secure(src: DeviceBuffer, dst: DeviceBuffer, stream: int = 0):
    """Middleware.Encode (Middleware.java:196-210) on the device."""
    N.check(N.lib().ipls_encode_secure(src.ptr, dst.ptr, min(src.n, dst.n), src.kind, dst.kind, stream or None))


def frame_parse(frame: bytes):
    """Header of a pubsub frame: (pid, n, a, b, payload_off, origin_off)."""
    a = np.frombuffer(bytes(frame), dtype=np.uint8)
    pid, x, y = ctypes.c_int16(), ctypes.c_int32(), ctypes.c_int32()
    po, oo = ctypes.c_int64(), ctypes.c_int64()
    n = N.check(N.lib().ipls_frame_parse(a.ctypes.data, a.size, ctypes.byref(pid), ctypes.byref(x),
                                         ctypes.byref(y), ctypes.byref(po), ctypes.byref(oo)))
    return pid.value, n, x.value, y.value, po.value, oo.value


def pair_parse(data):
    """Download_Partial_Updates (MyIPFSClass.java:326-338) through the C-ABI:
    (gradients as float64, workers, payload byte offset)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    w, off = ctypes.c_int32(), ctypes.c_int64()
    n = N.check(N.lib().ipls_pair_parse(a.ctypes.data, a.size, ctypes.byref(w), ctypes.byref(off)))
    g = np.frombuffer(a[off.value:off.value + 8 * n].tobytes(), dtype=">f8").astype(np.float64)
    return g, w.value, off.value


def pair_encode(workers: int, gradients) -> bytes:
    """ObjectOutputStream.writeObject(new Pair<>(workers, gradients)), as
    MyIPFSClass.Update_file(String, Pair) writes it (MyIPFSClass.java:160-166)."""
    g = np.ascontiguousarray(gradients, dtype=np.float64)
    n = N.check(N.lib().ipls_pair_encode(workers, g.ctypes.data, g.size, N.HOST_F64, None, 0))
    out = np.empty(n, dtype=np.uint8)
    N.check(N.lib().ipls_pair_encode(workers, g.ctypes.data, g.size, N.HOST_F64, out.ctypes.data, n))
    return out.tobytes()


def _u8(data) -> np.ndarray:
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _u8_ptr(a: np.ndarray):
    return ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_uint8)) if a.size else None


def parse_saved(data) -> dict[int, np.ndarray]:
    """DownloadMapParameters (MyIPFSClass.java:559-566) through the C-ABI: the
    HashMap<Integer,double[]> of a save_model file as {key: float64 array}, in
    the file's (HashMap iteration) order."""
    a = _u8(data)
    n = N.check(N.lib().ipls_saved_parse(a.ctypes.data, a.size, None, None, None, 0))
    keys = (ctypes.c_int32 * max(n, 1))()
    lens, offs = (ctypes.c_int64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))()
    N.check(N.lib().ipls_saved_parse(a.ctypes.data, a.size, keys, lens, offs, n))
    return {int(keys[i]): np.frombuffer(a[offs[i]:offs[i] + 8 * lens[i]].tobytes(), dtype=">f8").astype(np.float64)
            for i in range(n)}


def encode_saved(weights, order=None) -> bytes:
    """The bytes ObjectOutputStream writes for IPLS.save_model's map
    (IPLS.java:1904-1911): `weights` maps partition -> array, put in `order`
    (Auth_List; default: the mapping's own order)."""
    parts = [int(p) for p in (weights.keys() if order is None else order)]
    arrs = [np.ascontiguousarray(weights[p], dtype=np.float64) for p in parts]
    n = len(parts)
    cp = (ctypes.c_int32 * max(n, 1))(*parts)
    ca = (ctypes.c_void_p * max(n, 1))(*[x.ctypes.data for x in arrs])
    cl = (ctypes.c_int64 * max(n, 1))(*[x.size for x in arrs])
    need = N.check(N.lib().ipls_saved_encode(cp, n, ca, cl, N.HOST_F64, None, 0))
    out = np.empty(need, dtype=np.uint8)
    N.check(N.lib().ipls_saved_encode(cp, n, ca, cl, N.HOST_F64, out.ctypes.data, need))
    return out.tobytes()


def parse_darr(data) -> np.ndarray:
    """A serialised double[] (MyIPFSClass._Upload_File(double[], ...), :261-270)."""
    a = _u8(data)
    off = ctypes.c_int64()
    n = N.check(N.lib().ipls_darr_parse(a.ctypes.data, a.size, ctypes.byref(off)))
    return np.frombuffer(a[off.value:off.value + 8 * n].tobytes(), dtype=">f8").astype(np.float64)


def encode_darr(values) -> bytes:
    g = np.ascontiguousarray(values, dtype=np.float64)
    gp = _u8_ptr(g.view(np.uint8))
    n = N.check(N.lib().ipls_darr_encode(gp, g.size, N.HOST_F64, None, 0))
    out = np.empty(n, dtype=np.uint8)
    N.check(N.lib().ipls_darr_encode(gp, g.size, N.HOST_F64, out.ctypes.data, n))
    return out.tobytes()


def parse_dlist(data) -> np.ndarray:
    """DownloadParameters (MyIPFSClass.java:376-385): the values of a
    serialised ArrayList<Double>."""
    a = _u8(data)
    n = N.check(N.lib().ipls_dlist_parse(a.ctypes.data, a.size, None, 0))
    out = np.empty(n, dtype=np.float64)
    N.check(N.lib().ipls_dlist_parse(a.ctypes.data, a.size, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n))
    return out


def encode_dlist(values) -> bytes:
    """ObjectOutputStream.writeObject of an ArrayList<Double> (the `<ID>Model`
    and `<ID>ETHModel` files, IPLS.java:547-558, 2255-2273)."""
    g = np.ascontiguousarray(values, dtype=np.float64)
    gp = _u8_ptr(g.view(np.uint8))
    n = N.check(N.lib().ipls_dlist_encode(gp, g.size, N.HOST_F64, None, 0))
    out = np.empty(n, dtype=np.uint8)
    N.check(N.lib().ipls_dlist_encode(gp, g.size, N.HOST_F64, out.ctypes.data, n))
    return out.tobytes()


def frame_encode(gradient, a: int, b: int, pid: int, origin: bytes) -> bytes:
    """Marshall_Packet(double[],...) before base64 (MyIPFSClass.java:990-1017)."""
    if isinstance(gradient, DeviceBuffer):
        ptr, n, kind = gradient.ptr, gradient.n, N.DEV_F64
        keep = None
    else:
        keep = np.ascontiguousarray(np.zeros(0) if gradient is None else gradient, dtype=np.float64)
        ptr, n, kind = keep.ctypes.data, keep.size, N.HOST_F64
    o = np.frombuffer(bytes(origin), dtype=np.uint8)
    out = np.empty(14 + 8 * n + o.size, dtype=np.uint8)
    nb = N.check(N.lib().ipls_frame_encode(ptr, n, kind, a, b, pid, o.ctypes.data if o.size else None,
                                           o.size, out.ctypes.data, out.size))
    return out[:nb].tobytes()
