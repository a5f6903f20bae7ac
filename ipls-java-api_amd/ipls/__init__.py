"""ipls -- MI355X-native IPLS gradient-partition aggregation (host side).

The arithmetic runs in hand-written gfx950 HIP kernels inside
``ipls-java-api_amd/lib/libipls_agg.so`` behind the C-ABI of
``include/ipls_agg.h``; this package is the Python twin of the Java/JNI
binding plus the Middleware wire codec.
"""
from ._native import (  # noqa: F401
    ALL_PARTITIONS, DEV_BE, DEV_F64, DEV_TEXT, HOST_BE, HOST_BE_CANON, HOST_DARR, HOST_DLIST, HOST_F64, HOST_FRAME,
    HOST_PAIR, DEV_F32, HOST_F32, KERNEL_REDUCE_F32, DEV_F16, HOST_F16, DEV_BF16, HOST_BF16, KERNEL_REDUCE_H16,
    KERNEL_ROUND_F32, KERNEL_ROUND_H16, KERNEL_FOLD1_F32, KERNEL_FOLD1_H16, KERNEL_UPDATE_FLAT, KERNEL_ENCODE_FLAT,
    KERNEL_UPDATE_SEGS, KERNEL_DIVIDE_SEGS, KERNEL_ENCODE_SEGS, KERNEL_UPDATE_SEGS_DIFF, KERNEL_ENCODE_SEGS_DIFF,
    KERNEL_UPDATE_SEGS_PEERS, SEG_PEERS_MAX, KERNEL_DIVIDE_SEGS_COPIES, SEG_COPIES_MAX,
    KERNEL_ROUND_SEGS_PEERS,
    HOST_TEXT, KERNEL_FOLD1, KERNEL_REDUCE, KERNEL_REDUCE_SCALAR, KERNEL_ROUND, SHAPE_BIG, SHAPE_HALF, SHAPE_MID,
    SHAPE_SMALL, START_ACCUM, START_FIRST, START_ZERO, TGT_AGG, TGT_FUTURE, TGT_REP, TGT_WADDR, TGT_WEIGHTS,
    SAVED_BLEND, SAVED_SET, IplsError, build_info, lib,
)
from .aggregator import (  # noqa: F401
    Aggregator, DeviceBuffer, Difference, ModelCopies, PeerUpdates, PinnedBuffer, Segments, checksum_dev, encode_darr, encode_dlist, encode_saved, encode_secure,
    frame_encode, frame_parse, java_pair_hash, pair_encode, pair_parse, parse_darr, parse_dlist, parse_saved,
    shard_plan, synth_fill,
)

SEED = 0x1B5_2026  # synthetic workload seed
