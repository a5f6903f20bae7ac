/*
 * ipls_agg.h -- C-ABI of the MI355X-native IPLS gradient-partition aggregator.
 *
 * Drop-in boundary for the reference's aggregation path.
 * The reference has no FFI: its reduce loops are inlined into static-state
 * Java methods.  Each entry point below replaces the body of one of those
 * loops; the Java callers keep their signatures and call through the JNI
 * shim shown in INTEGRATION.md (1:1 mapping, no torch / HIP types here).
 *
 * Reference citations are relative to /root/reference/src/main/java/.
 *
 * Conventions
 *  - Every function returns IPLS_OK (0) or a negative IPLS_E_* code and never
 *    aborts; ipls_agg_last_error() gives the message (Java code catches and
 *    prints exceptions at the same places, e.g. Updater.java:213-215).
 *  - The caller owns host buffers for the duration of the call only: a call
 *    that reads or writes host memory has finished with it when it returns.
 *  - Calls with only device-resident operands are stream-ordered on the
 *    handle's HIP stream and may return before the GPU finishes; use
 *    ipls_agg_sync() before reading device results from another stream.
 *    The handle's stream is non-blocking: device operands written on another
 *    stream (the null stream included) must be complete, or ordered before
 *    the call by an event the handle's stream waits on (ipls_agg_stream /
 *    ipls_agg_partition_device give the stream).
 *  - A handle is internally serialised (one mutex per GPU shard): it may be
 *    called from the Updater thread and the daemon thread concurrently, as the
 *    Java code does under PeerData.mtx (PeerData.java:27).  Each CALL is one
 *    ordered unit: calls on one partition take effect in call order -- the
 *    reference's arrival order.  A SEQUENCE of calls is not a unit: another
 *    thread's call may land between two calls of one thread.  So what one
 *    Java-side step must do atomically is one call here: a whole arriving
 *    bucket (ipls_agg_accumulate, or ipls_agg_accumulate_chunked for a
 *    caller that produces the bucket chunk by chunk), AggregatePartition plus
 *    its commit_update bytes (ipls_agg_finalize, ipls_agg_finalize_chunked).
 *    A chunked call takes effect, as one unit, at one instant: an
 *    accumulate_chunked when its last chunk has landed on the GPU (as
 *    Middleware's Deserialize reads the whole stream before UpdateModel takes
 *    PeerData.mtx, Middleware.java:224, 246), a finalize_chunked /
 *    get_partitions(_wire)_chunked when it takes its snapshot, before the
 *    first chunk is delivered.  No shard lock is held while the caller's
 *    source or sink runs, so a blocking one (a socket) holds up nobody else.
 *    ipls_agg_accumulate_range / ipls_agg_read_range are single calls too:
 *    a caller that splits one arrival into ranges holds its own lock across
 *    them (PeerData.mtx, Updater.java:72-149) or gets a mixed order.
 *  - Every ipls_agg_* call returns with the calling thread's current HIP
 *    device unchanged, whichever GPUs the handle's shards live on.
 *  - Arithmetic is IEEE binary64 with no contraction and no reassociation:
 *    each element is folded over the peers in the order given, starting from
 *    +0.0 (or from the first bucket), so results are bit-identical to the
 *    Java loops on the same inputs.
 */
#ifndef IPLS_AGG_H
#define IPLS_AGG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPLS_AGG_ABI_VERSION 4

/* ---- error codes (Java exception the reference would raise) ---- */
#define IPLS_OK           0
#define IPLS_E_INVAL     -1  /* bad argument / null handle                         */
#define IPLS_E_RANGE     -2  /* partition index or length out of range
                                (ArrayIndexOutOfBoundsException, Updater.java:115) */
#define IPLS_E_NEGSIZE   -3  /* chunk rule gives a partition of length < 1
                                (NegativeArraySizeException, IPLS.java:1024,1863)  */
#define IPLS_E_NOMEM     -4  /* device or pinned-host allocation failed             */
#define IPLS_E_DEVICE    -5  /* HIP runtime / kernel launch error                   */
#define IPLS_E_FORMAT    -6  /* malformed frame or byte length
                                (BufferUnderflowException, MyIPFSClass.java:1444)  */
#define IPLS_E_NODEV     -7  /* no usable GPU                                       */

/* ---- accumulator targets (PeerData.java:137,144,149,189) ---- */
#define IPLS_TGT_AGG      0  /* PeerData.Aggregated_Gradients[p]  */
#define IPLS_TGT_REP      1  /* PeerData.Replicas_Gradients[p]    */
#define IPLS_TGT_WEIGHTS  2  /* PeerData.Weights[p]               */
#define IPLS_TGT_WADDR    3  /* PeerData.Weight_Address[p]        */
#define IPLS_TGT_FUTURE   4  /* PeerData.Aggregated_Gradients_from_future[p]
                                (Updater.java:99-101: a client's bucket for a
                                later iteration) */

/* ---- operand kinds ---- */
#define IPLS_HOST_F64     0  /* host double[] (native byte order)                          */
#define IPLS_HOST_BE      1  /* host byte[] of big-endian doubles: update_file / GetParameters
                                format (MyIPFSClass.java:105-116, 444-455); n = #doubles     */
#define IPLS_HOST_FRAME   2  /* host byte[] pubsub frame after base64 (Marshall_Packet,
                                MyIPFSClass.java:990-1017); n = frame byte length           */
#define IPLS_DEV_F64      3  /* device double*                                               */
#define IPLS_DEV_BE       4  /* device bytes, big-endian doubles, 8-byte aligned             */
#define IPLS_HOST_BE_CANON 5 /* output only: BE with NaN canonicalised, DataOutputStream
                                .writeDouble (Middleware.java:164-170)                      */
#define IPLS_HOST_PAIR    6  /* host byte[] of a Java-serialised org.javatuples.Pair<Integer,
                                double[]> partial update (MyIPFSClass.java:160-166, read by
                                Download_Partial_Updates :326-338); n = byte length         */
#define IPLS_HOST_TEXT    7  /* output only: host bytes of a base64url pubsub text
                                (Marshall_Packet's String, MyIPFSClass.java:1016)           */
#define IPLS_DEV_TEXT     8  /* output only: the same text in device memory                  */
#define IPLS_HOST_DARR    9  /* host byte[] of a Java-serialised double[] (the single-partition
                                hand-over file, MyIPFSClass.java:261-270); n = byte length  */
#define IPLS_HOST_DLIST  10  /* host byte[] of a Java-serialised ArrayList<Double> (`<ID>Model`,
                                `<ID>ETHModel`, IPLS.java:547-558, 2255-2273; read by
                                DownloadParameters, MyIPFSClass.java:376-385); n = byte
                                length; ipls_agg_load_model only                            */
/* The float32 trainer boundary.  The reference's trainer hands IPLS widened floats
 * (Model.java:423: Doubles.asList(gradient.getRow(0).toDoubleVector()) of a float INDArray)
 * and narrows what it takes back (Model.java:388-390: Dumm.put(0, j, arr.get(j)) before
 * model.setParams).  With these kinds the library does both on the device: a source is
 * read as floats, v = (double)src[i] (exact: signs, subnormals and NaNs as Java's
 * widening), then exactly what the F64 kind does -- so the bits are those of the F64 call
 * fed the widened values; an output is the F64 kind's value (the IEEE double quotient of
 * GetPartitions, secure mode included) rounded ONCE to float, ties to even (overflow to
 * +-inf, subnormal results kept, -0.0 kept): Java's (float)d.  n counts ELEMENTS.
 *   sources: ipls_agg_update_gradient, ipls_agg_split (src), ipls_agg_load_model,
 *            ipls_agg_accumulate, ipls_agg_accumulate_async (both kinds);
 *            ipls_agg_reduce_batch, ipls_agg_reduce_batch_out, ipls_agg_aggregate_round
 *            (bufs: DEV_F32; the destinations stay F64 / BE)
 *   outputs: ipls_agg_get_partitions (out_kind), ipls_agg_aggregate_round (avg_kind)
 *   streamed: ipls_agg_accumulate_chunked_narrow (HOST_F32 source),
 *            ipls_agg_get_partitions_chunked_narrow (HOST_F32 output); the JNI shim's
 *            float[] natives (accumulateFloats, getPartitionsFloats, updateGradientFloats,
 *            loadModelFloats) sit on these and on update_gradient / load_model
 * Every other call stays F64-only and refuses them with IPLS_E_INVAL like an unknown
 * kind: the F64 chunked calls (accumulate_chunked, finalize_chunked,
 * get_partitions(_wire)_chunked -- their trainer-format twins are the two _narrow calls
 * above), accumulate_range / read_range, the double[] / byte[] JNI natives, the BE, frame
 * and Java-serialised formats, set_weights, blend, other_replica, reduce_partial /
 * combine_partials, read, and the saved-model calls.  A count slot of an f32 bucket is
 * 1.0f.  A HOST_F32 operand crosses PCIe as 4 B per element (pinned ones too: they are
 * copied, not read zero-copy). */
#define IPLS_DEV_F32     11  /* device float*, 4-byte aligned                                 */
#define IPLS_HOST_F32    12  /* host float[] (native byte order)                              */
/* The half-precision trainer boundary: the same two lines of Model.java with a 2-byte
 * INDArray (a DL4J network built with DataType.HALF or BFLOAT16), or a PyTorch trainer
 * under autocast whose parameters and gradients are torch.float16 / torch.bfloat16.
 *   Sources (widening rule): v = (double)src[i], then exactly what the F64 kind does, so
 * the bits are those of the F64 call fed the widened values.  IEEE binary16 is widened
 * f16 -> f32 -> f64 (both steps exact, f16 subnormals kept); bfloat16 is (bits << 16) taken
 * as an f32, then -> f64 (exact; a bf16 subnormal is an f32 subnormal and is kept).  Signs
 * and +-0 are kept, infinities stay infinities, a quiet NaN gives a NaN (what a signalling
 * NaN's payload becomes is unspecified).  No flush-to-zero anywhere.
 *   Outputs (two-step narrowing rule): the IEEE double quotient of GetPartitions (secure
 * mode included) is FIRST rounded to float exactly as the F32 kind does (one round to
 * nearest even), THEN that float is rounded to the 16-bit format: ties to even, overflow
 * to +-inf, subnormal results kept, -0.0 stays -0.0, NaN stays a NaN.  So an F16 / BF16
 * output equals the F32 output narrowed by the trainer (numpy's astype(float16), torch's
 * .to(bfloat16)).  This is deliberately NOT a single rounding of the double: a quotient
 * of 1 + 2^-11 + 2^-30 gives the half 0x3c00 (a single rounding would give 0x3c01),
 * 1 + 2^-8 + 2^-30 the bfloat16 0x3f80 (not 0x3f81).  It is what a trainer gets today
 * when it narrows the F32 output itself, and it keeps the three output kinds consistent.
 *   n counts ELEMENTS; a count slot of a 16-bit bucket is 1.0 in that format.  The kinds
 * are accepted where the F32 kinds are and nowhere else:
 *   sources: ipls_agg_update_gradient, ipls_agg_split (src), ipls_agg_load_model,
 *            ipls_agg_accumulate, ipls_agg_accumulate_async (DEV and HOST kinds);
 *            ipls_agg_reduce_batch, ipls_agg_reduce_batch_out, ipls_agg_aggregate_round
 *            (bufs: the DEV kinds; the destinations stay F64 / BE)
 *   outputs: ipls_agg_get_partitions (out_kind), ipls_agg_aggregate_round (avg_kind)
 *   streamed: ipls_agg_accumulate_chunked_narrow, ipls_agg_get_partitions_chunked_narrow
 *            (the HOST kinds)
 * Every other call refuses them with IPLS_E_INVAL, as it refuses F32.  A HOST operand
 * crosses PCIe as 2 B per element (pinned ones too: copied, not read zero-copy). */
#define IPLS_DEV_F16     13  /* device IEEE binary16[], 2-byte aligned                        */
#define IPLS_HOST_F16    14  /* host IEEE binary16[] (native byte order)                      */
#define IPLS_DEV_BF16    15  /* device bfloat16[], 2-byte aligned                             */
#define IPLS_HOST_BF16   16  /* host bfloat16[] (native byte order)                           */

/* ---- ipls_agg_load_saved modes ---- */
#define IPLS_SAVED_SET    0  /* target[p] = file[p]                                          */
#define IPLS_SAVED_BLEND  1  /* target[p][i] = a*target[p][i] + b*file[p][i]  (Updater.java:65-69) */

/* ---- fold start modes ---- */
#define IPLS_START_ACCUM  0  /* fold into the target's current value (Updater arrival fold)     */
#define IPLS_START_ZERO   1  /* target = +0.0 first (fresh accumulator, IPLS.java:1888,1268)    */
#define IPLS_START_FIRST  2  /* target = bucket 0, then fold the rest
                                (Decentralized_Storage_Receiver.java:240-246)                   */

#define IPLS_ALL_PARTITIONS (-1)

typedef struct ipls_agg ipls_agg;

typedef struct ipls_agg_cfg {
    int64_t model_size;          /* PeerData._MODEL_SIZE; > 0 selects the reference chunk rule   */
    int32_t n_partitions;        /* -pa  (Middleware.java:35, PeerData._PARTITIONS)              */
    int32_t max_peers;           /* -n   (Middleware.java:44); sizes host staging, may be 0       */
    int32_t partial_aggregation; /* -aggr (Middleware.java:57); informational                     */
    int32_t secure;              /* PeerData.secure_ipls (PeerData.java:62): /1e12 in the divide  */
    int32_t device;              /* HIP device ordinal                                           */
    int32_t flags;               /* reserved, must be 0                                          */
    int64_t bucket_len;          /* model_size == 0: every partition has this length incl. the
                                    count slot (synthetic configs, SURVEY.md §8 notation)        */
    /* ABI 2: the devices of a multi-GPU handle (SURVEY.md §8(b) "device ids", §8(e)).
     * n_devices == 0 (or devices == NULL): one device, `device`.  Otherwise the
     * -pa partitions are sharded over devices[0..n_devices) in contiguous blocks,
     * partition p on shard p / ceil(P / n_devices) (ipls_shard_plan), each shard
     * with its own HIP stream and accumulator arena on its device; a device may
     * appear more than once (shards sharing one GPU).  The list is copied. */
    const int32_t *devices;
    int32_t n_devices;
    int32_t reserved;            /* must be 0 */
} ipls_agg_cfg;

/* Caller callbacks of the chunked calls (ipls_agg_get_partitions_chunked,
 * ipls_agg_finalize_chunked: sink; ipls_agg_accumulate_chunked: source).
 * They run on the calling thread, inside the call, with no library lock held:
 * they may block (a socket recv/send -- bound it with a timeout, the call
 * waits for its callback) and may call into the same handle. */
typedef int (*ipls_chunk_sink)(void *ctx, const double *values, int64_t offset, int64_t n);
typedef int (*ipls_chunk_source)(void *ctx, void *dst, int64_t offset, int64_t n);
/* The sink of ipls_agg_save_model_chunked: n bytes of the file at byte `offset`,
 * valid during the call only.  Same rules as ipls_chunk_sink.  (The prototype
 * spells the parameter IPLS_BYTE_SINK_FN *, the same type as ipls_byte_sink.) */
typedef int IPLS_BYTE_SINK_FN(void *ctx, const uint8_t *bytes, int64_t offset, int64_t n);
typedef IPLS_BYTE_SINK_FN *ipls_byte_sink;

/* ABI version of the loaded library (IPLS_AGG_ABI_VERSION). */
int ipls_agg_abi_version(void);

/* Allocate the per-partition accumulators on the device, all zero.
 * Replaces IPLS.init's InitializeWeights() (IPLS.java:1860-1878). */
int ipls_agg_open(const ipls_agg_cfg *cfg, ipls_agg **out);

/* Free everything.  NULL is accepted. */
int ipls_agg_close(ipls_agg *h);

/* Message of the last failure on h (h == NULL: last failure of this thread).
 * Right after a call fails, ipls_agg_last_error(NULL) is that call's message
 * even while other threads use the same handle.  The string belongs to the
 * calling thread and stays valid until its next ipls_agg_last_error call. */
const char *ipls_agg_last_error(const ipls_agg *h);

/* Partition length incl. the count slot: IPLS.java:1019-1028. */
int ipls_agg_partition_len(const ipls_agg *h, int p, int64_t *len);

/* Offset of partition p's first value in the flat model (p * chunk). */
int ipls_agg_partition_offset(const ipls_agg *h, int p, int64_t *off);
/* Values of the flat model: model_size (sum of L_p - 1), what GetPartitions
 * writes and OrganizeGradients reads. */
int ipls_agg_flat_size(const ipls_agg *h, int64_t *n);

/* InitializeWeights(List<Double> Model), IPLS.java:1880-1901: Weights and
 * Weight_Address get the model values with count slot 0.0; AGG, REP = 0.
 * src: HOST_F64 / HOST_BE (read_file format, IPLS.java:2000-2008) / DEV_* /
 * HOST_DLIST (n = byte length: the ArrayList<Double> that DownloadParameters
 * reads, IPLS.java:567; its element records are checked on the device before
 * anything is written, IPLS_E_FORMAT leaves every accumulator as it was). */
int ipls_agg_load_model(ipls_agg *h, const void *src, int64_t n, int src_kind);

/* OrganizeGradients (IPLS.java:1018-1040) for partition p: dst gets
 * double[L_p] with the count slot 1.0.  dst_kind: HOST_F64, HOST_BE, DEV_F64,
 * DEV_BE.  n is the length of the flat gradient vector. */
int ipls_agg_split(ipls_agg *h, const void *flat, int64_t n, int src_kind,
                   int p, void *dst, int dst_kind);

/* UpdateGradient's own-partition accumulate (IPLS.java:1737-1743):
 * for every p in owned[0..n_owned): AGG[p] = AGG[p] + OrganizeGradients(flat)[p].
 * flat == NULL is the "did not train in time" case (Gradients == null): no-op. */
int ipls_agg_update_gradient(ipls_agg *h, const void *flat, int64_t n, int src_kind,
                             const int32_t *owned, int n_owned);

/* Updater._Update for one arriving bucket (Updater.java:36-48 REP branch,
 * 74-137 AGG branches): target[p][i] = target[p][i] + g[i], i < L_p.
 * n = #doubles (F64/BE kinds) or frame byte length (FRAME kind; the frame's
 * n field must be >= L_p; PAIR kind: its double[] must be >= L_p).  Returns IPLS_E_RANGE when the bucket is shorter
 * than L_p.  Also Collect_Replicas (IPLS.java:1217-1241) with target REP.
 * DARR kind (n = byte length): like PAIR, its double[] must be >= L_p. */
int ipls_agg_accumulate(ipls_agg *h, int p, int target, const void *src, int64_t n,
                        int src_kind);

/* Asynchronous form of ipls_agg_accumulate (Updater._Update without waiting,
 * Updater.java:115-117); returns at once with *ticket.
 *  - DEV_F64 / DEV_BE (8-B aligned): the bucket is queued, not read.  Each
 *    partition's queued buckets are folded together in one launch, in call
 *    order (bit-identical to folding them one by one), when the queues fill
 *    (ipls_agg_set_coalesce, default 32), at ipls_agg_wait, or at the first
 *    other call on the handle.
 *  - pinned host memory (ipls_host_alloc, 16-B aligned, HOST_F64/HOST_BE):
 *    the fold is queued at once and reads the bucket over PCIe, so the next
 *    `ipfs cat` can fill another buffer meanwhile.
 *  - other sources run synchronously (ticket already done).
 * The caller keeps the bucket untouched (and allocated) until
 * ipls_agg_wait(h, ticket) -- or any other call on the handle -- returns.
 * Folds apply in call order. */
int ipls_agg_accumulate_async(ipls_agg *h, int p, int target, const void *src, int64_t n,
                              int src_kind, uint64_t *ticket);

/* One range of one arrival, asynchronous: src[0..n) is folded into
 * target[offset .. offset+n) of partition p (Agg[i] = Agg[i] + g[i],
 * Updater.java:115-117, for those i), reading pinned host memory
 * (ipls_host_alloc; HOST_F64 or HOST_BE) over PCIe with no staging copy.
 * offset must be even and src 16-B aligned.  A bucket folded as any set of
 * ranges that covers [0, L_p) once gets the bits of the whole-bucket fold:
 * every element is added once, in call order.  This lets a caller that must
 * first copy the bucket (the JNI shim's double[] natives) overlap that copy
 * with the fold, chunk by chunk.  Keep src untouched until
 * ipls_agg_wait(h, *ticket) returns.  IPLS_E_RANGE outside [0, L_p);
 * IPLS_E_INVAL for other memory or a misaligned range.
 * Each range is its own call: another thread's fold into the same target
 * can land between two ranges of one arrival, and the elements of the
 * earlier ranges then see a different order than those of the later ones.
 * Hold a lock across the ranges, or use ipls_agg_accumulate_chunked. */
int ipls_agg_accumulate_range(ipls_agg *h, int p, int target, const void *src, int64_t offset, int64_t n,
                              int src_kind, uint64_t *ticket);

/* One arriving bucket that the caller produces chunk by chunk, as ONE call
 * (Updater._Update's whole-bucket fold under PeerData.mtx, Updater.java:72-149,
 * 115-117): the library calls source(ctx, dst, offset, n) on the calling
 * thread for consecutive chunks of `chunk` values (even, >= 2) covering
 * [0, L_p); the source writes the bucket's values [offset, offset + n) into
 * dst -- 8 * n bytes of pinned staging owned by the library, native doubles
 * (HOST_F64) or big-endian bytes (HOST_BE) -- and returns 0.  Each chunk is
 * sent to the GPU while the source fills the next one; once every chunk has
 * landed, the bucket is folded into target[p] in one launch.
 *  - n is the caller's bucket length: n < L_p is IPLS_E_RANGE before any
 *    source call (the ArrayIndexOutOfBoundsException of Updater.java:115);
 *    values past L_p are never asked for.
 *  - All or nothing: a non-zero source return stops the call with
 *    IPLS_E_INVAL and nothing folded.
 *  - The chunks land in staging of this call's own, with no lock held; the
 *    shard's lock is taken once every chunk has landed, for the fold alone.
 *    So the bucket takes effect as one unit at that instant (a fold another
 *    thread makes into the same target while the source is still producing
 *    lands before it): the bits are those of ipls_agg_accumulate on the whole
 *    bucket at that point of the call order.  A slow source holds up no other
 *    caller of the shard.
 * The JNI shim's accumulate(double[]) source is GetDoubleArrayRegion; the
 * Middleware servers' is a socket recv. */
int ipls_agg_accumulate_chunked(ipls_agg *h, int p, int target, int64_t n, int src_kind, int64_t chunk,
                                ipls_chunk_source source, void *ctx);

/* ipls_agg_accumulate_chunked for a trainer's bucket: src_kind is HOST_F32,
 * HOST_F16 or HOST_BF16 (any other kind is IPLS_E_INVAL); n, chunk (even,
 * >= 2) and the source's offset / n count ELEMENTS, and the source writes
 * n * s bytes (s = 4 or 2) of the format into dst.  The values cross PCIe as
 * s bytes each and are widened in the fold (k_fold1_narrow from the call's
 * staging), so the bits are those of ipls_agg_accumulate(HOST_F32 / F16 /
 * BF16) on the whole bucket, i.e. of the F64 call fed the widened values.
 * Every rule of ipls_agg_accumulate_chunked holds word for word: no lock
 * while the source runs, the arrival takes effect as one unit when its last
 * chunk has landed, all or nothing, n < L_p is IPLS_E_RANGE before any source
 * call.  The JNI shim's accumulateFloats(float[]) sits on it. */
int ipls_agg_accumulate_chunked_narrow(ipls_agg *h, int p, int target, int64_t n, int src_kind, int64_t chunk,
                                       ipls_chunk_source source, void *ctx);

/* ipls_agg_update_gradient of one whole flat gradient that the caller produces
 * chunk by chunk, as ONE call: UpdateGradient over the owned partitions
 * (IPLS.java:1708-1743: OrganizeGradients splits everything, then the
 * accumulate loop runs) is one step of the reference, and this is its streamed
 * one-call form.  The bits are exactly those of ipls_agg_update_gradient on
 * the same vector.
 *  - src_kind is HOST_F64, HOST_BE, HOST_F32, HOST_F16 or HOST_BF16 (anything
 *    else is IPLS_E_INVAL): one entry point for all five.  n, chunk (even,
 *    >= 2) and the source's offset / n count ELEMENTS; the source writes
 *    count * s bytes (s = 8, 4 or 2) into dst, the library's pinned ring.
 *  - Every partition is bounds-checked first: a vector that overruns one
 *    (IPLS.java:1030) is IPLS_E_RANGE, an owned index outside [0, P) is
 *    IPLS_E_RANGE, a bad kind, chunk or a null source IPLS_E_INVAL -- all
 *    before any source call.  n_owned == 0 is a no-op with no source call.
 *  - For every owned p: AGG[p][i] = AGG[p][i] + v with v = (double)flat[off_p
 *    + i] for i < ncopy_p, 1.0 at i == ncopy_p (the count slot: generated by
 *    the kernel, it is not in the stream) and 0.0 above (the add is still
 *    made, so a -0.0 element becomes +0.0).  A logically-zero AGG is written
 *    as +0.0 + v without being read.  An index repeated in `owned` folds
 *    again, in a following launch.
 *  - Source calls: consecutive chunks, in order, covering [0, min(n, model
 *    size)), each at most `chunk` elements; on a multi-GPU handle a chunk never
 *    crosses the flat start of a shard, so the one before it is shorter.  The
 *    source is called for every chunk, also where no owned partition has
 *    values (a socket source must consume the stream); only the byte ranges of
 *    owned partitions cross PCIe, at most one copy per owned partition a
 *    chunk intersects.
 *  - Order: no lock is held while the source runs.  The whole gradient takes
 *    effect at one instant, after its last chunk has landed: the locks of the
 *    shards that hold an owned partition are taken in ascending shard index,
 *    all held at once, and under them each shard folds its queued arrivals,
 *    waits (on its stream) for its copies and gets one launch of
 *    k_update_flat over all its owned partitions.  That makes the gradient a
 *    unit against every other call on those shards: another call sees either
 *    none of it or all of it, in every partition.  It does not change the other
 *    calls: ipls_agg_get_partitions_chunked still snapshots shard after shard.
 *  - All or nothing: a non-zero source return gives IPLS_E_INVAL and leaves
 *    EVERY accumulator, zero flag and queue as it was, on every shard; the
 *    copies already queued are drained before the staging is reused.  The
 *    same holds for every refusal and for any failure before the first
 *    launch (a copy, an event, a staging allocation).  It does NOT hold for a
 *    device failure (IPLS_E_DEVICE: the job table's upload or a launch) on a
 *    later shard, or on the second launch of a repeated index, once an
 *    earlier launch has been issued: what that launch folded stays folded and
 *    its zero flags stay cleared, as after a device failure in any other call.
 *  - Memory: each involved shard stages its flat segment (up to the last owned
 *    value) times s bytes plus 32 bytes of padding in a device buffer of the
 *    call's own, pooled like the staging of the other chunked calls: the pool
 *    grows with the number of concurrent chunked calls and is freed only at
 *    close (it is not bounded). */
int ipls_agg_update_gradient_chunked(ipls_agg *h, int64_t n, int src_kind, const int32_t *owned, int n_owned,
                                     int64_t chunk, ipls_chunk_source source, void *ctx);

/* The reverse of a ranged fold, asynchronous: target[offset .. offset+n) of
 * partition p is copied into pinned host memory dst (ipls_host_alloc), as
 * doubles (HOST_F64) or as big-endian bytes (HOST_BE: putDouble order, what
 * update_file writes, MyIPFSClass.java:105-116).  dst is complete when
 * ipls_agg_wait(h, *ticket) returns.  With ipls_agg_finalize(h, p, NULL, ...)
 * first, reading IPLS_TGT_WEIGHTS in ranges gives the commit_update bytes
 * chunk by chunk -- but as separate calls, so a set_weights or a finalize
 * from another thread between them tears the bytes: ipls_agg_finalize_chunked
 * is the one-call form.  IPLS_E_RANGE outside [0, L_p); IPLS_E_INVAL for
 * other memory. */
int ipls_agg_read_range(ipls_agg *h, int p, int target, void *dst, int64_t offset, int64_t n, int dst_kind,
                        uint64_t *ticket);

/* Wait until fold `ticket` (and every fold queued before it) has finished. */
int ipls_agg_wait(ipls_agg *h, uint64_t ticket);

/* Launch the folds of every queued asynchronous device bucket now, without
 * waiting for them (for example when the Updater's queue runs dry). */
int ipls_agg_flush(ipls_agg *h);

/* Coalescing group g (>= 1; 1 = fold each arrival at once) of asynchronous
 * device buckets: the queues are flushed when they average g buckets per
 * partition or one of them holds 2g.  Device traffic per element is
 * (g + 2) * 8 bytes for a group of g buckets, against 24 * g one by one. */
int ipls_agg_set_coalesce(ipls_agg *h, int max_group);

/* Updater.run's indirect request (Updater.java:176-187): the queue item holds
 * only a hash, so the bucket is `ipfs cat` bytes read into the Updater's one
 * reusable Gradient_Buff of (int)M/P + 2 doubles (Updater.java:162, zeroed
 * once) by GetParameters(hash, Gradient_Buff) (MyIPFSClass.java:444-455), and
 * _Update folds Gradient_Buff[0..L_p) into target[p].  Exactly as in Java, a
 * file shorter than L_p leaves the tail of the previous request in the buffer
 * and that tail is folded; a file longer than the buffer overwrites the
 * buffer, folds nothing and returns IPLS_E_RANGE (the AIOOBE).  The handle
 * owns the buffer (one per handle, like one Updater thread per peer). */
int ipls_agg_update_indirect(ipls_agg *h, int p, int target, const void *bytes, int64_t n_bytes);

/* ---- PeerData.Other_Replica_Gradients (PeerData.java:140-141) ----
 * The downloads of OTHER aggregators' buckets of partition p, kept per key
 * (p, aggregator) in a java.util.HashMap<Pair<Integer,String>, double[]>.
 *
 * The aggregator index contract.  The reference key is the aggregator's
 * peer-ID String.  Here `aggregator` is any int32 the caller maps 1:1 from
 * that String (e.g. its index in the Java side's table of known peers, or an
 * interned ID): two keys are the same key exactly when (p, aggregator) are
 * equal.  `key_hash` is the reference key's hashCode,
 *     new org.javatuples.Pair<>(p, peerId).hashCode()
 * (Java computes it directly; ipls_java_pair_hash computes it from the ID's
 * UTF-8 bytes).  It fixes where the key sits in the HashMap, and so the order
 * in which Collect_Replicas folds the stored arrays: floating-point addition
 * does not associate, so that order decides the bits of REP[p] once a
 * partition has two or more stored arrays.  ipls_agg_other_replica (no hash)
 * takes the peer ID to be Integer.toString(aggregator). */

/* new Pair<Integer,String>(p, id).hashCode() (javatuples 1.2, pom.xml:66-68) of a
 * peer ID given as UTF-8 bytes: 31 + 31*(31 + p) + id.hashCode() in wrapping
 * int32 arithmetic, String.hashCode over the ID's UTF-16 units.  IPLS_E_FORMAT
 * for malformed UTF-8.  No handle, no GPU. */
int ipls_java_pair_hash(int32_t p, const uint8_t *id, int64_t len, int32_t *hash);

/* Download_Scheduler.download_gradients, a bucket of ANOTHER aggregator of
 * partition p (Download_Scheduler.java:245-268): kept per (p, aggregator) in
 * Other_Replica_Gradients -- the first download becomes the stored array
 * (its own length n, -0.0 kept) and the key is put into the map model with
 * key_hash; later ones fold into it for j < n and leave its position as it
 * is (a later call with another key_hash for a stored key: IPLS_E_INVAL).  A
 * later download longer than the stored array returns IPLS_E_RANGE, nothing
 * folded.  Other_Replica_Gradients_Received counts the downloads. */
int ipls_agg_other_replica_keyed(ipls_agg *h, int p, int32_t aggregator, int32_t key_hash, const void *src,
                                 int64_t n, int src_kind);
/* The same with the peer ID Integer.toString(aggregator). */
int ipls_agg_other_replica(ipls_agg *h, int p, int32_t aggregator, const void *src, int64_t n,
                           int src_kind);

/* Other_Replica_Gradients.remove(new Pair<>(p, aggregator)) and the same
 * remove on Other_Replica_Gradients_Received: the stored array and its
 * download count are discarded (the HashMap keeps its capacity).  Returns 1
 * if the key was stored, 0 if not (no-op).  The reference removes the key when
 * that aggregator's own partial sum has arrived, so its downloaded buckets
 * are not counted twice: Download_Scheduler.java:215-217 (already in
 * Received_Replicas), :329-332 and :438-440 (its partial-update file
 * downloaded).  GlobalGradientPool.java:90-93 builds its key from the
 * frame's List<String> of origins, which never equals a stored
 * Pair<Integer,String>: that remove is a no-op in the reference
 * (INTEGRATION.md §2). */
int ipls_agg_other_replica_drop(ipls_agg *h, int p, int32_t aggregator);

/* Collect_Replicas (IPLS.java:1217-1241): REP[p][j] = REP[p][j] + Other[(p,a)][j]
 * for every stored key, in the order of new ArrayList<>(keySet()) of the JDK
 * HashMap (ascending bin of the key hashes under the map's capacity, then
 * insertion order within a bin), then clears the store
 * (Other_Replica_Gradients = new HashMap<>(): capacity reset).
 * participants (nullable, P ints) receives, per partition, what the reference
 * adds to PeerData.Participants[p]: its put / replace sits inside the element
 * loop (IPLS.java:1229-1234), so every stored key adds its download count
 * (Other_Replica_Gradients_Received) once per element -- received * length,
 * wrapping like Java int.  The Java side adds a nonzero entry to its map
 * (put if absent, else +=).  Returns the number of stored arrays folded, or
 * IPLS_E_RANGE (nothing folded) if one is longer than its partition. */
int ipls_agg_collect_replicas(ipls_agg *h, int32_t *participants);

/* The order Collect_Replicas would fold the stored keys in right now, as
 * (partition, aggregator) pairs: pairs[2i], pairs[2i+1].  Returns the number
 * of stored keys and writes the first min(that, max_pairs) of them (pairs may
 * be NULL with max_pairs 0 to ask for the count); a return above max_pairs
 * means the list was cut -- another thread may have stored keys since the
 * count was asked for -- and the caller asks again with more room.
 * A diagnostic for a Java caller to check the library's HashMap model against
 * its own `new ArrayList<>(Other_Replica_Gradients.keySet())`.  *capacity
 * (nullable) receives the model's table capacity (0 after new HashMap<>()). */
int ipls_agg_replica_order(ipls_agg *h, int32_t *pairs, int max_pairs, int32_t *capacity);

/* Batched fixed-order fold, ONE kernel launch for n_parts partitions:
 *   for q in [0,n_parts): target[p_first+q] = fold(start_mode; bufs[q*k + 0..k-1])
 * bufs are device pointers (DEV_F64 or DEV_BE), each at least L_p long.
 * This is the benchmarked kernel. */
int ipls_agg_reduce_batch(ipls_agg *h, int p_first, int n_parts,
                          const void *const *bufs, int k, int src_kind,
                          int start_mode, int target);

/* The same batched fold written to caller device buffers, one per partition
 * (dst[q], at least L_p doubles / 8*L_p bytes): dst_kind DEV_BE fuses the
 * double->byte pack of update_file (MyIPFSClass.java:105-116) into the fold,
 * src_kind DEV_BE the byte->double unpack of GetParameters (:444-455).  With
 * START_FIRST this is the storage node's `-aggr 1` merge
 * (Decentralized_Storage_Receiver.java:239-258: S = g0; S += g_i; write the
 * `_partial_aggregation` file).  ACCUM reads dst in dst_kind's byte order. */
int ipls_agg_reduce_batch_out(ipls_agg *h, int p_first, int n_parts,
                              const void *const *bufs, int k, int src_kind,
                              int start_mode, void *const *dst, int dst_kind);

/* Pubsub ingest on the device (ThreadReceiver.run/process, IPLS.java:851-866,
 * 399-465; Utils.getRawMessage, Utils.java:8-17).  msgs[i] / lens[i] are the
 * JSON "data" texts of n_msgs pubsub messages: `layers` (1 or 2) rounds of
 * java.util.Base64 URL encoding of a Marshall_Packet frame
 * (MyIPFSClass.java:990-1017).  They are copied to the device, decoded there
 * (alphabet and '=' rules of Base64.getUrlDecoder), parsed as GET_GRADIENTS
 * frames (MyIPFSClass.java:1437-1459), and each payload is folded (BE decode
 * fused) into target[p] in message order.  p = parts[i], or the frame's
 * partition field when parts is NULL.  A bad message is dropped and reported,
 * as the Java receiver drops it after printing the exception:
 * status[i] = 0 folded, 1 null gradient (n == 0, no fold), IPLS_E_FORMAT
 * (bad base64 / short frame), IPLS_E_RANGE (partition out of range or
 * payload shorter than L_p).  Returns the number of messages folded.
 * The texts are copied by IPLS_INGEST_COPY_THREADS (default 2) short-lived
 * host threads, each on its own stream, while the device decodes the texts
 * that have already landed; msgs must stay valid until the call returns. */
int ipls_agg_ingest_pubsub(ipls_agg *h, int target, const uint8_t *const *msgs,
                           const int64_t *lens, int n_msgs, int layers,
                           const int32_t *parts, int32_t *status);

/* Variants (-async true / leaving peers):
 *   blend: target[p][i] = a*target[p][i] + b*g[i]  (products rounded, then the sum)
 *     async replica fold  a = 0.75, b = 1        Updater.java:57-59
 *     leaving-peer blend  a = 0.6,  b = 1 - 0.6  Updater.java:65-69
 *   scale: dst[p][i] = c * src[p][i]             Updater.java:197-199 (0.25 * W)
 * blend also takes HOST_DARR (n = byte length; one partition of a leaving
 * peer); ipls_agg_load_saved blends a whole saved-model file. */
int ipls_agg_blend(ipls_agg *h, int p, int target, const void *src, int64_t n, int src_kind,
                   double a, double b);
int ipls_agg_scale(ipls_agg *h, int p, int dst_target, int src_target, double c);

/* AggregatePartition (IPLS.java:1248-1274): W = AGG + REP, Weight_Address = W,
 * AGG = REP = 0.  p may be IPLS_ALL_PARTITIONS.  Optional host outputs for one
 * partition: sum_out (the commit_update file bytes, IPLS_Comm.java:27-37 ->
 * update_file, when sum_kind == HOST_BE; or doubles, HOST_F64) and avg_out
 * (L_p - 1 averaged values, the GetPartitions divide).  Either may be NULL. */
int ipls_agg_finalize(ipls_agg *h, int p, void *sum_out, int sum_kind, double *avg_out);

/* ipls_agg_finalize of one partition with its sum handed to a sink chunk by
 * chunk, as ONE call: AggregatePartition (IPLS.java:1248-1274), then W[p]
 * comes back through a pinned ring (three slots) in chunks of `chunk` values
 * (even, >= 2), sink(ctx, values, offset, n) on the calling thread for
 * consecutive ranges of [0, L_p), so the sink's copy of one chunk overlaps
 * the transfer of the next.  values: n 8-byte values, doubles (HOST_F64) or
 * the commit_update file bytes (HOST_BE, update_file's putDouble order,
 * MyIPFSClass.java:105-116), valid during the sink call only.  Under the
 * shard's lock the call runs AggregatePartition and snapshots W (or its
 * bytes) into staging of its own; the lock is released before the first sink
 * call.  So the bytes are this call's W whatever set_weights, fold or
 * finalize another thread makes meanwhile (never torn), and a slow sink
 * holds up nobody.  A non-zero sink return stops the delivery with
 * IPLS_E_INVAL; the round is consumed either way (W is written, AGG = REP =
 * 0), as after a failed update_file.  The JNI shim's finalizePartition(byte[])
 * sink is SetByteArrayRegion. */
int ipls_agg_finalize_chunked(ipls_agg *h, int p, int sum_kind, int64_t chunk, ipls_chunk_sink sink, void *ctx);

/* A whole aggregation round for partitions [p_first, p_first+n_parts) in ONE
 * kernel launch (one pass over the buckets):
 *   AGG[p]   = AGG[p] + b_0 + ... + b_{k-1}     Updater._Update folds (Updater.java:115-117)
 *   W[p]     = AGG[p] + REP[p]; AGG = REP = 0   AggregatePartition (IPLS.java:1248-1274)
 *   avg_out  = W[p][j] / W[p][L_p-1]            GetPartitions divide (IPLS.java:1159-1174)
 * AGG is never stored: its final value only feeds W.  Results are bit-identical
 * to reduce_batch(ACCUM) + finalize + get_partitions.  bufs: n_parts*k device
 * buckets (DEV_F64/DEV_BE, or the trainer kinds DEV_F32/DEV_F16/DEV_BF16; k
 * may be 0).  avg_out (or NULL) receives the averaged values of the
 * partitions, partition p at flat offset partition_offset(p) -
 * partition_offset(p_first) -- for all partitions the GetPartitions model;
 * avg_kind DEV_F64 or HOST_F64, or a DEV/HOST F32, F16 or BF16 kind (the
 * narrowing rules of those kinds).
 * What runs fused (one launch after a one-wave-per-partition count pre-pass),
 * every bucket 16-B aligned:
 *   DEV_F64 / DEV_BE buckets, avg_out NULL or DEV_F64 / HOST_F64   (k_round)
 *   DEV_F32 / DEV_F16 / DEV_BF16 buckets, avg_out NULL or any of the six
 *   trainer kinds, bucket and average formats free to differ   (k_round_narrow)
 * What takes the three steps (the fold into AGG, AggregatePartition, the
 * divide) inside the call, with the same bits: a bucket off a 16-B boundary;
 * trainer-format buckets with F64 averages; F64 / BE buckets with
 * trainer-format averages.  A HOST avg_kind adds one device-to-host copy. */
int ipls_agg_aggregate_round(ipls_agg *h, int p_first, int n_parts,
                             const void *const *bufs, int k, int src_kind,
                             void *avg_out, int avg_kind);

/* Download_Scheduler.cache_partition (Download_Scheduler.java:752-792):
 * Weight_Address[p] = GetParameters(hash) -- the downloaded updated partition
 * (n doubles, F64/BE host or device kinds).  src_kind HOST_FRAME (n = frame
 * bytes) is the pid-4 ACK of ThreadReceiver (IPLS.java:491-498): the frame's
 * first L_p payload doubles become Weight_Address[p].  HOST_DARR (n = byte
 * length): the serialised double[]'s values, under the GetParameters rule. */
int ipls_agg_set_weights(ipls_agg *h, int p, const void *src, int64_t n, int src_kind);

/* GetPartitions (IPLS.java:1140-1174): Weights = Weight_Address, then the
 * flat model with every partition divided by its count slot (count 0.0 ->
 * values unchanged; secure -> / (1e12 * count)).  out holds model_size
 * doubles; out_kind HOST_F64, HOST_BE_CANON (Middleware task-3 stream), DEV_F64. */
int ipls_agg_get_partitions(ipls_agg *h, void *out, int64_t n, int out_kind);

/* GetPartitions (IPLS.java:1159-1174) delivered in chunks of `chunk` doubles
 * (even, >= 2) to sink(ctx, values, offset, n) on the calling thread, in
 * model order: the divide runs once on the GPU into staging of this call's
 * own -- every shard's, each under its shard lock for that launch only,
 * before any chunk is delivered, so the whole model is one snapshot -- then
 * each chunk comes back through a pinned ring (three slots) with no lock held, so
 * the sink's copy of chunk k overlaps the transfer of chunk k + 1 (the JNI
 * getPartitions(double[]) copies each chunk into the Java array with
 * SetDoubleArrayRegion).  `values` is valid only during the sink call.  A
 * non-zero sink return stops the transfer: the call returns IPLS_E_INVAL and
 * no further chunk is delivered.  Replaces the same loop as
 * ipls_agg_get_partitions. */
int ipls_agg_get_partitions_chunked(ipls_agg *h, int64_t chunk, ipls_chunk_sink sink, void *ctx);

/* ipls_agg_get_partitions_chunked with the model narrowed to a trainer
 * format on the GPU: out_kind is HOST_F32, HOST_F16 or HOST_BF16 (any other
 * kind is IPLS_E_INVAL), and the values are exactly those of
 * ipls_agg_get_partitions with that kind (one rounding of the double quotient
 * to float, then for the 16-bit kinds the second rounding).  The snapshot is
 * model_size * s bytes (s = 4 or 2); `chunk` counts ELEMENTS (even, >= 2);
 * the sink gets BYTES: sink(ctx, bytes, offset, n) with `offset` and `n` in
 * bytes of the flat narrowed model, every piece a whole number of elements.
 * Multi-shard handles snapshot every shard first and deliver in model order.
 * Other rules as ipls_agg_get_partitions_chunked.  The JNI shim's
 * getPartitionsFloats(float[]) sits on it. */
int ipls_agg_get_partitions_chunked_narrow(ipls_agg *h, int out_kind, int64_t chunk,
                                           IPLS_BYTE_SINK_FN *sink, void *ctx);

/* The same delivery as Middleware task 3's reply (Serialize, Middleware.java:
 * 164-170): each chunk is n values of the writeDouble stream -- big-endian
 * bytes, NaN canonicalised, written by the divide kernel -- so a socket sink
 * sends chunk k while chunk k + 1 comes back over PCIe (ipls.middleware's
 * loopback server).  Rules as ipls_agg_get_partitions_chunked. */
int ipls_agg_get_partitions_wire_chunked(ipls_agg *h, int64_t chunk, ipls_chunk_sink sink, void *ctx);

/* Copy an accumulator out (tests, replica publish IPLS.java:1423-1431).
 * dst_kind HOST_F64, HOST_BE, DEV_F64, DEV_BE; n >= L_p. */
int ipls_agg_read(ipls_agg *h, int p, int target, void *dst, int64_t n, int dst_kind);

/* End of IPLS.Update_Client_WaitAck_List (IPLS.java:1556-1562): for every p
 * in parts[0..n_parts): AGG[p] = FUTURE[p]; FUTURE[p] = 0.  O(1) per partition
 * (the two accumulators swap storage), so an address from ipls_agg_device_ptr
 * for AGG or FUTURE of such a p is stale afterwards. */
int ipls_agg_promote_future(ipls_agg *h, const int32_t *parts, int n_parts);

/* Zero AGG[p] and REP[p] (IPLS.java:1268-1269); p may be IPLS_ALL_PARTITIONS. */
int ipls_agg_reset(ipls_agg *h, int p);

/* Device address of an accumulator (for RCCL send/recv of replica partials).
 * Work the caller orders on the handle's stream sees the folds of every call
 * made so far -- except device buckets still queued by
 * ipls_agg_accumulate_async: call ipls_agg_flush (or any other entry point)
 * before reading the accumulator through this address. */
int ipls_agg_device_ptr(ipls_agg *h, int p, int target, void **ptr);

/* The handle's HIP stream (hipStream_t as void*) and a host wait on it
 * (ipls_agg_sync also folds queued device buckets first). */
void *ipls_agg_stream(ipls_agg *h);
int ipls_agg_sync(ipls_agg *h);

/* Order-independent checksum of partition p of a target:
 *   sum_i splitmix64(bits(x_i) + i*0x9E3779B97F4A7C15) mod 2^64
 * computed on the device (wave DPP + LDS reduction, exact integer sum). */
int ipls_agg_checksum(ipls_agg *h, int p, int target, uint64_t *out);

/* ---- multi-GPU (cfg.devices) ----
 * A partition's accumulators live on its owner shard.  Its contributors may
 * span GPUs the way the reference's replica aggregators of one partition do
 * (IPLS.java:1402-1468: each aggregator folds the buckets it received, the
 * partials are published at :1423-1431, the owner adds them in
 * Collect_Replicas :1449 / the Updater replica branch, Updater.java:40-44,
 * and AggregatePartition :1462-1468 forms W = AGG + REP).  Here a replica
 * aggregator is a SLOT: a shard other than the owner folds the buckets
 * resident on its GPU into the slot's partial sum of p
 * (ipls_agg_reduce_partial), and ipls_agg_combine_partials pulls the partials
 * of every other slot over xGMI (peer loads in the owner's fold kernel) and
 * folds them into REP[p] in ascending slot order:
 *     REP[p] = ((REP[p] + R_s1) + R_s2) + ...     (REP starts at +0.0)
 * which is the reference's expression for aggregators s1 < s2 < ...  */

/* Owner shard of partition p: its HIP device ordinal and stream (hipStream_t
 * as void*; work on p's device pointers is ordered on that stream).  Either
 * output may be NULL. */
int ipls_agg_partition_device(ipls_agg *h, int p, int32_t *device, void **stream);

/* The contiguous-block shard plan of cfg.devices, without a handle (no GPU
 * needed): owner[p] = p / ceil(n_partitions / n_shards) for every p. */
int ipls_shard_plan(int32_t n_partitions, int32_t n_shards, int32_t *owner);

/* Replica slot `slot` (a shard index, not the owner of any partition in
 * range) folds k device buckets per partition -- resident on that slot's
 * device -- into its partial sums of partitions [p_first, p_first+n_parts):
 *     R_slot[p] = fold(start_mode; bufs[q*k + 0..k-1])
 * with the same kernels and order as ipls_agg_reduce_batch.  ACCUM folds on
 * top of the slot's current partial (+0.0 after a combine). */
int ipls_agg_reduce_partial(ipls_agg *h, int slot, int p_first, int n_parts, const void *const *bufs, int k,
                            int src_kind, int start_mode);

/* For every partition of [p_first, p_first+n_parts): REP[p] += the partial of
 * every slot that folded into p since the last combine, slots ascending, in
 * one launch per owner shard that reads the partials over xGMI (partitions
 * with the same number of live slots share a launch whichever GPUs hold their
 * partials, so an owner reads over all its links at once); the partials are
 * then logically +0.0 again.  Returns the number of partials folded.
 * A pair of devices without peer access is not an error: such a partial is
 * first copied into an owner-side buffer (hipMemcpyPeerAsync on the SLOT's
 * stream, after the slot's folds, so copies from different GPUs run at once;
 * the partial's `ready` event is then re-recorded on that stream and the
 * owner waits on it) and the same fold reads that copy, in the same slot
 * order, so the result is bit-identical.  Memory: each such owner-side
 * buffer is L_p doubles per (slot, partition) pair that was ever staged,
 * allocated on the owner at the first staged combine and kept until
 * ipls_agg_close -- up to (G-1) extra copies of every partition an owner
 * holds on a node without peer access; it is not reserved at open, so an
 * out-of-memory shows up as IPLS_E_NOMEM from this call.  Setting
 * IPLS_PEER_STAGED=1 in the environment before ipls_agg_open forces this
 * path for every cross-shard read (the combine and the Gradient_Buff of
 * ipls_agg_update_indirect) -- a test switch; ipls_launch_info.staged counts
 * the staged partials.  The staged path has run only with shards sharing one
 * GPU (a copy within one device); between two distinct GPUs it is unmeasured
 * on hardware. */
int ipls_agg_combine_partials(ipls_agg *h, int p_first, int n_parts);

/* ---- publish-side codec (a9) ----
 * Marshall_Packet(target[p], origin, a, b, pid) (MyIPFSClass.java:990-1016),
 * as the aggregator publishes its partial sum every round
 * (IPLS.java:1429-1430: a = middleware_iteration, b = workers + 1, pid = 3):
 * the frame [i16 pid][i32 L_p][i32 a][i32 b][L_p x f64 BE][origin] encoded
 * with Base64.getUrlEncoder ('=' padding), produced on the device straight
 * from the accumulator (k_b64url_encode_frame).  origin = the bytes of
 * OriginPeer.getBytes() the frame carries (String.length() of them).
 * out_kind IPLS_HOST_TEXT (copied back, call complete on return) or
 * IPLS_DEV_TEXT (device buffer, stream-ordered).  Returns the text length
 * 4*ceil((14 + 8*L_p + origin_len)/3); out == NULL: the length only. */
int64_t ipls_agg_publish_partial(ipls_agg *h, int p, int target, int32_t a, int32_t b, int16_t pid,
                                 const uint8_t *origin, int32_t origin_len, void *out, int64_t out_cap,
                                 int out_kind);

/* The same for several partitions in one launch per GPU: the publish loop
 * over Auth_List (IPLS.java:1423-1431), text i = Marshall_Packet(target[
 * parts[i]], origin, a, b[i], pid) base64url-encoded.  Text i lands at
 * out + offs[i] (offs are 64-byte multiples, texts in list order), lens[i]
 * bytes.  lens/offs (n_parts entries, either may be NULL) are filled even
 * when out == NULL.  Returns the bytes the buffer needs (offs[n-1] +
 * lens[n-1]); b and origin may be NULL when out is (origin_len still counts).  IPLS_DEV_TEXT with partitions on several GPUs: out must be
 * memory every owner device can write (its own or a peer's). */
int64_t ipls_agg_publish_partials(ipls_agg *h, const int32_t *parts, int n_parts, int target, int32_t a,
                                  const int32_t *b, int16_t pid, const uint8_t *origin, int32_t origin_len,
                                  void *out, int64_t out_cap, int out_kind, int64_t *lens, int64_t *offs);

/* ---- send-side codec ----
 * The sender's half of a round: every peer is a client for the partitions it
 * does not own and sends each of them its slice of the gradient, every round.
 * Text i is produced on the device straight from the flat vector
 * (k_b64url_encode_flat, one launch per GPU): no split to host doubles, no
 * host frame, no host base64 pass.
 *
 * The frame is [i16 pid][i32 L_p][i32 parts[i]][i32 iteration][L_p x f64 BE]
 * [origin].  With lo = the partition's flat offset and ncopy = the values of
 * flat that fall into it (OrganizeGradients, IPLS.java:1018-1040), payload
 * value j is
 *   (double)flat[lo + j]  for j < ncopy: the widening rules of the F32 / F16 /
 *                         BF16 kinds above; doubles pass bit for bit (HOST_BE /
 *                         DEV_BE: their bytes as they are);
 *   1.0                   at j == ncopy, the count slot (IPLS.java:1033);
 *   +0.0                  for ncopy < j < L_p (a vector shorter than the model).
 * No addition is made anywhere: putDouble writes raw bits, so a -0.0 value is
 * -0.0 in the text (unlike ipls_agg_update_gradient, whose +0.0 + -0.0 is
 * +0.0), and a NaN keeps its payload.
 *
 * src_kind: exactly the kinds of ipls_agg_split (HOST / DEV x F64, BE, F32,
 * F16, BF16), with its refusals; from host memory only the bytes from the
 * first listed partition's first value to the last one's last value cross
 * PCIe.  As in OrganizeGradients every partition of the model is bounded
 * first: a vector that overruns any partition is IPLS_E_RANGE before anything
 * is written, and so is a listed index outside [0, P).  flat == NULL is the
 * "did not train in time" send (IPLS.java:1306-1312): every text is
 * Marshall_Packet(null, ...), n = 0, the header and the origin.
 *
 * The text is ONE base64 layer, what Marshall_Packet returns; the second layer
 * that receivers undo first (ipls_agg_ingest_pubsub, layers = 2) is the pubsub
 * transport's own.  Secure mode's Middleware.Encode is not applied: a secure
 * caller encodes before it sends (ipls_encode_secure), as Middleware.java:242-
 * 244 does before UpdateModel.
 *
 * The call reads and writes no accumulator and does not fold queued
 * asynchronous arrivals.  Text layout, out == NULL (sizes only), lens / offs,
 * the 64-byte text offsets, out_kind and stream ordering: as
 * ipls_agg_publish_partials.  IPLS_DEV_TEXT or a DEV source with partitions
 * on several GPUs: memory every owner device can reach. */
/* SendGradients (IPLS.java:1350-1400 -> Send_Gradient_Partition :1290-1322, direct mode): text i =
 * Base64.getUrlEncoder(Marshall_Packet(OrganizeGradients(flat)[parts[i]], origin, parts[i], iteration, pid)) */
int64_t ipls_agg_send_gradients(ipls_agg *h, const void *flat, int64_t n, int src_kind,
                                const int32_t *parts, int n_parts, int32_t iteration, int16_t pid,
                                const uint8_t *origin, int32_t origin_len,
                                void *out, int64_t out_cap, int out_kind, int64_t *lens, int64_t *offs);

/* ---- the trainer boundary over a LIST of arrays (no flat copy in or out) ----
 *
 * A trainer's model is a list of parameter tensors, its gradient a list of
 * separately allocated arrays, often of mixed precision.  A SEGMENT LIST is
 * n_segs device arrays (ptrs[s], ns[s] elements, kinds[s]); kinds[s] is
 * IPLS_DEV_F64, IPLS_DEV_F32, IPLS_DEV_F16 or IPLS_DEV_BF16, mixed freely.
 * The flat vector it stands for is the concatenation of the segments in list
 * order (parameters_to_vector order, each array read in memory order), of
 * n = sum of ns[s] values; value f is (double)ptrs[s][f - start_s], widened by
 * the rule stated above for that kind.  Everything after that is what the flat
 * call does with that vector:
 *   ipls_agg_update_gradient_segs  the accumulators end with the bits of
 *       ipls_agg_update_gradient(IPLS_DEV_F64) fed the widened concatenation
 *       (count slot 1.0 generated, +0.0 above it, the add always made);
 *   ipls_agg_send_gradients_segs   the texts of ipls_agg_send_gradients fed
 *       the same (a -0.0 stays -0.0, the count slot is generated);
 *   ipls_agg_get_partitions_segs   element f of the OUTPUT list is what
 *       ipls_agg_get_partitions writes at f for that segment's kind: doubles
 *       as they are, F32 one rounding of the IEEE double quotient, F16 / BF16
 *       the two-step rule; zero-count passthrough and secure mode included.
 * The list: a zero-length segment is legal and holds nothing (its pointer is
 * not looked at); n_segs == 0 is a vector of NO values -- not the null
 * gradient, which keeps going through the flat calls; every pointer of a
 * non-empty segment must be non-NULL and aligned to its element size, else
 * IPLS_E_INVAL naming the segment; host kinds, BE kinds, unknown kinds and a
 * negative length are IPLS_E_INVAL.  Input segments may alias each other;
 * overlapping output segments are the caller's problem.
 * Order of checks and effects, exactly the flat twins': every partition of the
 * model is bounded first (a list whose n overruns a partition is IPLS_E_RANGE
 * with nothing written on any shard; for get_partitions_segs n < the flat size
 * is IPLS_E_RANGE, and values beyond the model size are not written), then the
 * owned / partition list is checked, then the segments, and only then comes
 * the first launch.  Locking, the fold of queued arrivals before an update and
 * stream ordering of device outputs are those of ipls_agg_update_gradient,
 * ipls_agg_send_gradients and ipls_agg_get_partitions with a DEV kind.  On a
 * handle over several GPUs each shard takes the part of the list that meets
 * its flat segment; every array a shard touches must be memory its device can
 * reach (IPLS_E_DEVICE otherwise, before anything is written).
 * send_gradients_segs with out == NULL returns the sizes only. */
int ipls_agg_update_gradient_segs(ipls_agg *h, const void *const *ptrs, const int64_t *ns, const int32_t *kinds,
                                  int n_segs, const int32_t *owned, int n_owned);
int64_t ipls_agg_send_gradients_segs(ipls_agg *h, const void *const *ptrs, const int64_t *ns, const int32_t *kinds,
                                     int n_segs, const int32_t *parts, int n_parts, int32_t iteration, int16_t pid,
                                     const uint8_t *origin, int32_t origin_len,
                                     void *out, int64_t out_cap, int out_kind, int64_t *lens, int64_t *offs);
int ipls_agg_get_partitions_segs(ipls_agg *h, void *const *ptrs, const int64_t *ns, const int32_t *kinds, int n_segs);

/* ---- the trainer's update as the DIFFERENCE of two lists ----
 *
 * What the reference trainer hands to UpdateModel is GetDiff(model.params(),
 * Dumm) (Model.java:413, body :126-128) = Dumm.sub(model.params()):
 * Difference(received_model, trained_params), element by element, the
 * subtraction made in the arrays' own data type and only the result widened.
 * A DIFFERENCE LIST is a segment list with two pointer tables over one ns /
 * kinds table: a_ptrs[s] the minuend, b_ptrs[s] the subtrahend, lengths and
 * kinds equal by construction.  Value f = start_s + e of the flat vector it
 * stands for is (double) sub_k(a[s][e], b[s][e]):
 *   IPLS_DEV_F64          the IEEE double a - b;
 *   IPLS_DEV_F32          the float a - b, rounded once to float, then widened
 *                         exactly; a subnormal result is kept (no flush);
 *   IPLS_DEV_F16, _BF16   (float)a - (float)b in float, rounded to
 *                         nearest-even into the format, then widened by the
 *                         rule of that kind; subnormals are kept, a half
 *                         result beyond +-65504 is +-inf (what torch.sub and
 *                         numpy's float16 subtraction give).
 * x - x is +0.0; (-0.0) - (+0.0) is -0.0 and stays -0.0 in a text; a NaN the
 * subtraction makes (inf - inf) is a NaN like any other.  No contraction, no
 * fast-math.  The library takes no side on which list is "the model".
 *   ipls_agg_update_gradient_segs_diff  the accumulators end with the bits of
 *       ipls_agg_update_gradient(IPLS_DEV_F64) fed the widened difference;
 *   ipls_agg_send_gradients_segs_diff   the texts of ipls_agg_send_gradients
 *       fed the same vector.
 * Everything else is the _segs twins', word for word: count slot and zero
 * tail, order of checks (wherever a list is looked at, the minuend list, then
 * the subtrahend list), all-or-nothing on every shard, locking, the fold of
 * queued arrivals before an update, stream ordering, out == NULL for the sizes
 * only, n_segs == 0 as the vector of no values; on a handle over several GPUs
 * every array of EITHER list that a shard touches must be memory its device
 * can reach (IPLS_E_DEVICE before anything is written).  A NULL b_ptrs with
 * n_segs > 0 is IPLS_E_INVAL; a NULL or misaligned pointer of a non-empty
 * segment in either list is IPLS_E_INVAL, the message naming the segment and
 * the list ("minuend" / "subtrahend").  The two lists may alias each other and
 * themselves.  Pairs of different kinds, host lists and a difference OUTPUT
 * list do not exist. */
int ipls_agg_update_gradient_segs_diff(ipls_agg *h, const void *const *a_ptrs, const void *const *b_ptrs,
                                       const int64_t *ns, const int32_t *kinds, int n_segs,
                                       const int32_t *owned, int n_owned);
int64_t ipls_agg_send_gradients_segs_diff(ipls_agg *h, const void *const *a_ptrs, const void *const *b_ptrs,
                                          const int64_t *ns, const int32_t *kinds, int n_segs,
                                          const int32_t *parts, int n_parts, int32_t iteration, int16_t pid,
                                          const uint8_t *origin, int32_t origin_len,
                                          void *out, int64_t out_cap, int out_kind, int64_t *lens, int64_t *offs);

/* ---- K trainers' lists folded in one call ----
 *
 * The reference's documented experiment is many trainers against one machine
 * (Model.java:98-105; remote_fit and the Computational_Server, Model.java:134-
 * 140, 407-410, exist to make that bearable).  On one GPU that is K models of
 * one architecture side by side, all trained from the same received model.
 * A PEER LIST is n_peers segment lists over one ns / kinds table, lengths and
 * kinds equal by construction: t_ptrs[k * n_segs + s] is peer k's array of
 * segment s (peer-major).  Peer k's flat value f = start_s + e is
 *   m_ptrs == NULL   (double) t_k[s][e]: K plain lists;
 *   m_ptrs != NULL   (double) sub_kind(m[s][e], t_k[s][e]): the one shared
 *                    minuend list (the received model) minus trainer k's
 *                    parameters, the subtraction made in the segment's own
 *                    format exactly as the _segs_diff calls define it.
 * The accumulators, their logically-zero states and the count slots end with
 * the bits of calling ipls_agg_update_gradient_segs(t_k) -- or
 * ipls_agg_update_gradient_segs_diff(a_ptrs = m_ptrs, b_ptrs = t_k) -- once
 * per peer, for k = 0 .. n_peers - 1 in that order, with the same `owned`:
 * a partition owned once gets (((start + v_0) + v_1) + ..) + v_{K-1}, start =
 * +0.0 where the accumulator is logically zero; its count slot is added 1.0
 * K times, one after another; the tail above it +0.0 K times (a -0.0 there
 * becomes +0.0).  Nothing on the peer axis is reassociated.  A partition
 * listed r times in `owned` gets each peer's value added r times in a row
 * before the next peer's (the bits of K calls whose repeat levels run inside
 * each call).  Queued arrivals of a shard are folded before anything of this
 * call, as by a single ipls_agg_update_gradient.  The whole call is one
 * ordered unit: one hold of each involved shard's lock, one launch per shard,
 * all or nothing -- every check runs before the first launch on any shard, in
 * the twins' order: geometry (every partition bounded: IPLS_E_RANGE), `owned`,
 * then the lists, the minuend first, then peers 0 .. K-1.
 * n_peers < 1, n_peers > IPLS_SEG_PEERS_MAX and a NULL t_ptrs are
 * IPLS_E_INVAL; a NULL or misaligned pointer of a non-empty segment is
 * IPLS_E_INVAL, the message naming the segment and the list ("minuend" /
 * "peer k"); kinds and lengths as for the _segs calls.  On a handle over
 * several GPUs every array of ANY list that a shard touches must be memory its
 * device can reach (IPLS_E_DEVICE before anything is written).  n_segs == 0 is
 * the vector of no values, K times.  The lists may alias each other, the
 * minuend included.  n_peers == 1 is this call's own kernel too, not the
 * twin's (ipls_agg_last_launch says IPLS_KERNEL_UPDATE_SEGS_PEERS).
 * What does not exist: per-peer minuends, pairs of different kinds, host
 * lists, a send twin (each simulated peer's texts carry its own origin), JNI
 * and C++ mirrors, and a cache of plans between calls. */
#define IPLS_SEG_PEERS_MAX 1024
int ipls_agg_update_gradient_segs_peers(ipls_agg *h,
                                        const void *const *m_ptrs,   /* n_segs minuend pointers, or NULL */
                                        const void *const *t_ptrs,   /* n_peers * n_segs, peer-major */
                                        int n_peers,
                                        const int64_t *ns, const int32_t *kinds, int n_segs,
                                        const int32_t *owned, int n_owned);

/* ---- GetPartitions into K trainers' lists in one call ----
 *
 * The way back out of the many-trainers round: after it every one of the K
 * trainers must hold the new model in its own parameter arrays, and so must
 * the shared received model (the minuend of the next round's _segs_peers
 * call).  An OUTPUT COPY LIST is n_lists segment lists over one ns / kinds
 * table, lengths and kinds equal by construction: o_ptrs[k * n_segs + s] is
 * list k's array of segment s (list-major), the device of the peer list.
 * For every k, element f of list k ends with the bits that
 * ipls_agg_get_partitions_segs writes when given list k alone: doubles stored
 * as they are, F32 one rounding of the IEEE double quotient, F16 / BF16 the
 * two-step rule, zero-count passthrough, secure mode's 1e12 * cnt divisor,
 * values beyond the model size left unwritten, zero-length segments holding
 * nothing (their pointers are not looked at).  W and the count slots are read
 * once and the division is made once.  The whole call is one ordered unit: one
 * hold of each involved shard's lock -- every list receives the same W,
 * whatever another thread's aggregate or cache_partition does meanwhile --
 * and one launch per shard, all or nothing: every check runs before the first
 * launch on any shard, in the twin's order: the table, n < the flat size
 * (IPLS_E_RANGE), then lists 0 .. n_lists - 1 (a NULL or misaligned pointer of
 * a non-empty segment is IPLS_E_INVAL, the message naming the segment and
 * "list k"; kinds and lengths as for the _segs calls), and on a handle over
 * several GPUs every array of EVERY list that a shard touches must be memory
 * its device can reach (IPLS_E_DEVICE).  A refusal writes nothing to any list.
 * n_lists < 1, n_lists > IPLS_SEG_COPIES_MAX and a NULL o_ptrs with n_segs > 0
 * are IPLS_E_INVAL.  Lists that overlap each other are the caller's problem,
 * as overlapping output segments are for the twin.  n_lists == 1 is this
 * call's own kernel too, not the twin's (ipls_agg_last_launch says
 * IPLS_KERNEL_DIVIDE_SEGS_COPIES).  Stream ordering, and on a handle over
 * several GPUs the snapshot taken shard after shard, are the twin's.
 * What does not exist: lists of different kinds per copy, host lists, JNI and
 * C++ mirrors, and a cache of plans between calls. */
#define IPLS_SEG_COPIES_MAX 1025          /* IPLS_SEG_PEERS_MAX trainers + the received model */
int ipls_agg_get_partitions_segs_copies(ipls_agg *h,
                                        void *const *o_ptrs,         /* n_lists * n_segs, list-major */
                                        int n_lists,
                                        const int64_t *ns, const int32_t *kinds, int n_segs);

/* ---- the many-trainers round over tensor lists in one call ----
 *
 * What closes an iteration of the many-trainers experiment on one GPU: the K
 * trainers' lists folded, AggregatePartition of the owned partitions, and the
 * new model written back into every trainer's arrays.  The end state -- W,
 * the accumulators' logically-zero states, the count slots and every output
 * list -- is, bit for bit, that of these three steps made under ONE hold of
 * each shard's lock:
 *   1. ipls_agg_update_gradient_segs_peers(h, m_ptrs, t_ptrs, n_peers, ns,
 *      kinds, n_segs, owned, n_owned);
 *   2. ipls_agg_finalize(h, p, NULL, 0, NULL) for every distinct p in `owned`;
 *   3. ipls_agg_get_partitions_segs_copies(h, o_ptrs, n_lists, ns, kinds,
 *      n_segs).
 * A partition in `owned`: queued arrivals of its shard are folded first; the
 * fold is (((start + v_0) .. mult times) + v_1 ..) + v_{K-1}, start = +0.0
 * where AGG is logically zero, the count-slot and tail rules the peer-list
 * call's; W = that + REP by exactly k_finalize's operation (REP logically
 * zero: an addition of +0.0, so a -0.0 sum becomes +0.0); AGG and REP are left
 * in place and flagged logically zero -- AGG is never stored.  A partition
 * not in `owned`: W is read only.  Every partition: each list k gets
 * narrow_kind(W[i] / W[L_p - 1]) by the output-copy-list call's rules (always
 * the IEEE double division, one rounding to F32, the two-step rule for F16 /
 * BF16, zero-count passthrough, secure mode's 1e12 * cnt, nothing at or past
 * the model size).  The count a partition is divided by is its final count
 * slot: for an owned one ((AGG_slot or +0.0) + 1.0 added K * mult times one
 * after another) + REP_slot.
 * ALIASING is part of the contract: an output list may be the very arrays of
 * the minuend list or of any peer list -- the same pointer for the same
 * segment of the same table -- which is the main use (the trainers' own
 * parameters and the received model take the new model in place).  Every
 * read the call makes of an element happens before any write of it, and the
 * result is the one computed from the values before the call.  Any other
 * overlap between an output and an input or another output is the caller's
 * problem.
 * Every check runs before the first launch on any shard, and a refusal leaves
 * every accumulator, flag, queued arrival, W and list byte as it was:
 * n_peers outside [1, IPLS_SEG_PEERS_MAX], n_lists outside
 * [1, IPLS_SEG_COPIES_MAX], a NULL t_ptrs, a NULL o_ptrs with n_segs > 0
 * (IPLS_E_INVAL); then the peer-list call's checks in its order (geometry,
 * `owned`, the minuend, peers 0 .. K-1); then the output-copy-list call's
 * (n < the flat size is IPLS_E_RANGE, then lists 0 .. n_lists-1, the messages
 * naming the segment and "list k"); then, on a handle over several GPUs, that
 * every array of every list a shard touches is memory its device can reach
 * (IPLS_E_DEVICE).  Both bounds together leave n == the flat size.
 * n_owned == 0 is the divide into the lists alone.  n_peers == 1 and
 * n_lists == 1 run this call's own kernel too (ipls_agg_last_launch says
 * IPLS_KERNEL_ROUND_SEGS_PEERS).  On a handle over several GPUs the shards
 * are taken one after another, each shard's part under one hold of its lock
 * and in one launch; the model-wide snapshot caveat is the output-copy-list
 * call's.
 * What does not exist: per-list dtypes, host lists, a fused send, JNI and C++
 * mirrors, and a cache of plans between calls. */
int ipls_agg_round_segs_peers(ipls_agg *h,
                              const void *const *m_ptrs,   /* n_segs minuend pointers (the received model), or NULL */
                              const void *const *t_ptrs,   /* n_peers * n_segs, peer-major */
                              int n_peers,
                              void *const *o_ptrs,         /* n_lists * n_segs, list-major */
                              int n_lists,
                              const int64_t *ns, const int32_t *kinds, int n_segs,
                              const int32_t *owned, int n_owned);

/* ---- observability ----
 * What the last fold launch of a handle (of p's shard for multi-GPU handles:
 * the shard of the last call) ran: the kernel, the tile shape chosen by the
 * dispatch, lanes per workgroup, 16-B vectors per lane per
 * tile, the SEQ schedule code, the block->tile map and the grid. */
#define IPLS_KERNEL_REDUCE        1  /* k_reduce        */
#define IPLS_KERNEL_ROUND         2  /* k_round (fused) */
#define IPLS_KERNEL_FOLD1         3  /* k_fold1         */
#define IPLS_KERNEL_REDUCE_SCALAR 4  /* k_reduce_scalar */
#define IPLS_KERNEL_REDUCE_F32    5  /* k_reduce_narrow over DEV_F32 buckets; a tile is block x 4 x vectors
                                        elements; shape 0; seqf 1 when every operand was 16-B
                                        aligned (vector path), 0 for the element-by-element form */
#define IPLS_KERNEL_REDUCE_H16    6  /* k_reduce_narrow over DEV_F16 / DEV_BF16 buckets; a tile is block x 4 x
                                        vectors elements; shape 0; seqf 1 when every operand was 16-B
                                        aligned (vector path), 0 for the element-by-element form */
#define IPLS_KERNEL_ROUND_F32     7  /* k_round_narrow (fused) over DEV_F32 buckets; a tile is block x 4 x
                                        vectors elements; shape 0; seqf 1; map 3 (partial tiles first) or 0 */
#define IPLS_KERNEL_ROUND_H16     8  /* k_round_narrow (fused) over DEV_F16 / DEV_BF16 buckets; as above */
#define IPLS_KERNEL_FOLD1_F32     9  /* k_fold1_narrow: one F32 arrival (accumulate, accumulate_chunked_narrow),
                                        pointers as kernel arguments; block lanes, `vectors` groups of 4
                                        elements per lane in flight, a block's trip is 4 x block x vectors
                                        elements, grid-stride over `grid` blocks; shape 0; seqf 1 */
#define IPLS_KERNEL_FOLD1_H16    10  /* k_fold1_narrow: one F16 / BF16 arrival; as above */
#define IPLS_KERNEL_UPDATE_FLAT  11  /* k_update_flat (update_gradient_chunked): one launch over a shard's owned
                                        partitions; a tile is block x 2 x vectors doubles or block x 4 x vectors
                                        trainer-format elements; grid = blocks x jobs; shape 0; seqf 1 when
                                        every job had a full tile of values (the vector body), else 0; start
                                        ZERO when every job's accumulator was logically zero, else ACCUM */
#define IPLS_KERNEL_ENCODE_FLAT  12  /* k_b64url_encode_flat (send_gradients): one launch over a shard's listed
                                        partitions; a lane writes the 32 chars of 24 frame bytes, a fast lane from
                                        `vectors` = 4 source elements; grid = blocks x jobs; shape 0; seqf 1 when
                                        at least one lane of one job took the fast path, else 0; be_in as for the
                                        fold kernels */
/* The segment-list kernels: block x vectors is the tile in elements, laid over the destination, the same for
 * every element format; grid is the blocks (items) of the call's last launch.  (Enumerators, not macros: the
 * macro list above is the set of kernels of the flat vector calls, which stays as it is.) */
enum {
    IPLS_KERNEL_UPDATE_SEGS = 13,    /* k_update_segs (update_gradient_segs): one launch per shard and repeat
                                        level, one block per accumulator tile; seqf 1 when at least one block
                                        took the vector body (a full tile inside one segment), else 0; start as
                                        for IPLS_KERNEL_UPDATE_FLAT */
    IPLS_KERNEL_DIVIDE_SEGS = 14,    /* k_divide_segs (get_partitions_segs): one block per tile of an output
                                        segment (its head up to the first 128-B line is a block of its own);
                                        seqf 1 when at least one block took the vector body */
    IPLS_KERNEL_ENCODE_SEGS = 15,    /* k_b64url_encode_segs (send_gradients_segs): as IPLS_KERNEL_ENCODE_FLAT;
                                        a lane writes the text of 24 frame bytes = `vectors` = 3 payload values;
                                        seqf 1 when at least one lane had its four values in one segment */
    IPLS_KERNEL_UPDATE_SEGS_DIFF = 16, /* k_update_segs_diff (update_gradient_segs_diff): every field as for
                                        IPLS_KERNEL_UPDATE_SEGS */
    IPLS_KERNEL_ENCODE_SEGS_DIFF = 17, /* k_b64url_encode_segs_diff (send_gradients_segs_diff): every field as for
                                        IPLS_KERNEL_ENCODE_SEGS */
    IPLS_KERNEL_UPDATE_SEGS_PEERS = 18,/* k_update_segs_peers (update_gradient_segs_peers): one launch per shard
                                        whatever `owned` repeats; every field as for IPLS_KERNEL_UPDATE_SEGS */
    IPLS_KERNEL_DIVIDE_SEGS_COPIES = 19,/* k_divide_segs_copies (get_partitions_segs_copies): one launch per shard
                                        whatever n_lists; every field as for IPLS_KERNEL_DIVIDE_SEGS */
    IPLS_KERNEL_ROUND_SEGS_PEERS = 20  /* k_round_segs_peers (round_segs_peers): one launch per shard, one block per
                                        tile of EVERY partition of the shard, owned or not; seqf as for
                                        IPLS_KERNEL_UPDATE_SEGS; start ZERO when every owned partition's AGG was
                                        logically zero, else ACCUM; 0 when nothing is owned (the divide alone) */
};
#define IPLS_SHAPE_BIG    1
#define IPLS_SHAPE_MID    2
#define IPLS_SHAPE_SMALL  3
#define IPLS_SHAPE_HALF   4  /* 512 lanes x 16 vectors: native doubles, few partitions */
typedef struct ipls_launch_info {
    int32_t kernel, shape, block, vectors, seqf, map;
    int64_t grid;
    int32_t be_in, be_out, start;
    int32_t staged;   /* partials the handle's last ipls_agg_combine_partials copied to the owner
                         first (no xGMI peer access, or IPLS_PEER_STAGED=1) instead of peer loads */
} ipls_launch_info;
int ipls_agg_last_launch(ipls_agg *h, ipls_launch_info *out);

/* ---- host memory ---- */

/* Pinned host memory for IPFS byte buffers / the Middleware stream (the Java
 * side wraps it with JNI NewDirectByteBuffer).  Host operands that live in
 * such memory are DMA'd to the device directly, without a staging copy. */
int ipls_host_alloc(size_t bytes, void **ptr);
/* (Such buffers are also valid DEV_F64 / DEV_BE bucket pointers for
 * ipls_agg_reduce_batch: the fold kernel then reads them over PCIe directly,
 * zero copy.  ipls_agg_accumulate does this by itself for pinned sources.) */
int ipls_host_free(void *ptr);

/* ---- device utilities (no handle) -- stream may be NULL (default stream) ---- */

/* Fill a device bucket with the synthetic workload of SURVEY.md §8(d):
 * x_i = (2u-1)*1e-2, u = (splitmix64(seed ^ p<<40 ^ k<<32 ^ i) >> 11) * 2^-53,
 * x_{L-1} = 1.0 (count slot).  dst_kind DEV_F64 or DEV_BE. */
int ipls_synth_fill(void *dst, int64_t len, uint64_t seed, int p, int k, int dst_kind,
                    void *stream);

/* Checksum (as above) of n device doubles (DEV_F64) or BE doubles (DEV_BE). */
int ipls_checksum_dev(const void *src, int64_t n, int src_kind, uint64_t *out, void *stream);

/* Middleware.Encode (secure mode, Middleware.java:196-210) on n device
 * doubles: clip to +-10 then scale by 1e12 (dst may equal src). */
int ipls_encode_secure(const void *src, void *dst, int64_t n, int src_kind, int dst_kind,
                       void *stream);

/* Pubsub frame header parse (MyIPFSClass.java:1437-1446 / 1462-1469).
 * Returns the number of doubles n, or IPLS_E_FORMAT. */
int64_t ipls_frame_parse(const uint8_t *frame, int64_t len, int16_t *pid, int32_t *a,
                         int32_t *b, int64_t *payload_off, int64_t *origin_off);

/* Frame encode (MyIPFSClass.java:990-1017) of n device or host doubles into a
 * host byte buffer of 14 + 8n + origin_len bytes.  Returns bytes written. */
int64_t ipls_frame_encode(const double *g, int64_t n, int g_kind, int32_t a, int32_t b,
                          int16_t pid, const uint8_t *origin, int32_t origin_len,
                          uint8_t *out, int64_t out_cap);

/* ---- the partial-update object: Java-serialised Pair<Integer, double[]> ----
 * IPLS_Comm.commit_partial_update (IPLS_Comm.java:51-61) and
 * DStorage_Client.sendPartition(..., mod 1) (DStorage_Client.java:152-154,
 * `-i 1`) write new Pair<>(workers, Aggregated_Gradients[p]) with
 * ObjectOutputStream; Download_Scheduler (:324-325) and the storage merge
 * (Decentralized_Storage_Receiver.java:249-256) read it back. */

/* Parse such a stream: returns the number of doubles (the payload is that
 * many big-endian doubles at byte *payload_off) and the Integer in *workers,
 * or IPLS_E_FORMAT (not a Pair<Integer,double[]> object stream, or truncated). */
int64_t ipls_pair_parse(const uint8_t *buf, int64_t len, int32_t *workers, int64_t *payload_off);

/* The exact bytes ObjectOutputStream.writeObject(new Pair<>(workers, g)) writes
 * for n doubles (g_kind HOST_F64 or HOST_BE).  Returns the byte count; with
 * out == NULL only the count; IPLS_E_RANGE if out_cap is too small. */
int64_t ipls_pair_encode(int32_t workers, const void *g, int64_t n, int g_kind, uint8_t *out,
                         int64_t out_cap);

/* commit_partial_update's file bytes for AGG[p] (IPLS.java:1423-1425):
 * Pair<>(workers, Aggregated_Gradients[p]) with the payload packed on the
 * device.  Returns the byte count (out == NULL: count only). */
int64_t ipls_agg_commit_partial(ipls_agg *h, int p, int32_t workers, uint8_t *out, int64_t out_cap);

/* The storage node's merge (Decentralized_Storage_Receiver.java:239-258) of k
 * downloaded files: status 0 -> raw BE files (file_kind HOST_BE), status != 0
 * -> Pair partial updates (HOST_PAIR).  Aggregation = the first file's doubles;
 * then Aggregation[j] += g[j] for j < g.length, file by file; the result is
 * written to out as the `<p>_partial_aggregation` file bytes (update_file: BE).
 * Returns the byte count; IPLS_E_RANGE when a later file is longer than the
 * first (the reference's ArrayIndexOutOfBoundsException) or out_cap is short. */
int64_t ipls_agg_merge_files(ipls_agg *h, const uint8_t *const *files, const int64_t *lens, int k,
                             int file_kind, uint8_t *out, int64_t out_cap);

/* ---- saved-model files: Java-serialised weight maps and lists ----
 * JDK 8 ObjectOutputStream streams that carry whole weight partitions between
 * peers:
 *   MAP    HashMap<Integer,double[]> of Weights[p] for p in Auth_List: IPLS.terminate
 *          -> save_model (IPLS.java:1981-1998, 1904-1911); the peer that takes a
 *          partition over reads it with DownloadMapParameters (MyIPFSClass.java:
 *          559-566, IPLS.java:728-731) and the Updater blends it in (Updater.java:65-69)
 *   DARR   a bare double[]: the single-partition hand-over (MyIPFSClass.java:261-270,
 *          IPLS.java:136-140)
 *   DLIST  ArrayList<Double> of the whole model: IPLS_HOST_DLIST above
 * double[] payloads keep the raw bits of every value; the boxed Doubles of a
 * DLIST go through Double.doubleToLongBits, so every NaN becomes
 * 0x7ff8000000000000 (the IPLS_HOST_BE_CANON rule).  Both rules are read from
 * the JDK 8 sources; no JVM was at hand to pin them.
 * Entries of a MAP come in java.util.HashMap iteration order (Integer.hashCode()
 * is the value; table of 16 doubling past 0.75 * capacity). */

/* Host-only codecs (no handle, no GPU), mirrors of ipls_pair_parse / _encode.
 * Parsers accept exactly the shapes the JDK writes and never read past len;
 * anything else is IPLS_E_FORMAT with the reason in ipls_agg_last_error(NULL).
 *
 * ipls_saved_parse: a MAP.  Returns the entry count and fills the first
 * min(count, max_entries) rows: key, array length, byte offset of the array's
 * big-endian payload (any of the three may be NULL).  Duplicate keys are
 * IPLS_E_FORMAT. */
int64_t ipls_saved_parse(const uint8_t *bytes, int64_t len, int32_t *keys, int64_t *lens, int64_t *payload_offs,
                         int64_t max_entries);
/* The MAP of `n_parts` arrays: keys parts[i] put in that order (a key listed
 * twice keeps its first position and its first array), arrays[i] of lens[i]
 * values (g_kind HOST_F64 or HOST_BE).  Returns the byte count; out == NULL:
 * the count only; IPLS_E_RANGE if out_cap is too small. */
int64_t ipls_saved_encode(const int32_t *parts, int n_parts, const void *const *arrays, const int64_t *lens, int g_kind,
                          uint8_t *out, int64_t out_cap);
/* A DARR: returns the array length, its payload at byte *payload_off (27). */
int64_t ipls_darr_parse(const uint8_t *bytes, int64_t len, int64_t *payload_off);
int64_t ipls_darr_encode(const void *g, int64_t n, int g_kind, uint8_t *out, int64_t out_cap);
/* A DLIST: returns the element count; values (nullable, max_values doubles)
 * receives the first min(count, max_values) of them after every element
 * record has been checked. */
int64_t ipls_dlist_parse(const uint8_t *bytes, int64_t len, double *values, int64_t max_values);
int64_t ipls_dlist_encode(const void *g, int64_t n, int g_kind, uint8_t *out, int64_t out_cap);

/* save_model (IPLS.java:1904-1911): the MAP of target[p] for p in parts
 * (Auth_List, in its order; duplicates as ipls_saved_encode), every payload
 * packed on the device.  target is normally IPLS_TGT_WEIGHTS.  Returns the
 * byte count; out == NULL: the count only. */
int64_t ipls_agg_save_model(ipls_agg *h, const int32_t *parts, int n_parts, int target, uint8_t *out, int64_t out_cap);

/* The same file handed to a sink piece by piece, as ONE call: each shard packs
 * its entries into a staging of this call's own under that shard's lock, every
 * lock is released before the first sink call, then the pieces -- consecutive,
 * in stream order, each at most chunk_bytes (>= 16) long -- come back through
 * the pinned ring.  A non-zero sink return stops the delivery with
 * IPLS_E_INVAL.  Rules as ipls_agg_finalize_chunked; the sink may call into
 * the handle.  On a multi-GPU handle the shards are snapshotted one after the
 * other, and the staging pool is unbounded, as for the other chunked calls. */
int ipls_agg_save_model_chunked(ipls_agg *h, const int32_t *parts, int n_parts, int target, int64_t chunk_bytes,
                                IPLS_BYTE_SINK_FN *sink, void *ctx);

/* The DARR file of target[p] (IPLS.java:136-140). */
int64_t ipls_agg_save_partition(ipls_agg *h, int p, int target, uint8_t *out, int64_t out_cap);

/* The DLIST of target[p][0..L_p) for p = 0..P-1 in order: the loops at
 * IPLS.java:549-555 and 2255-2260 (count slots included, as there). */
int64_t ipls_agg_save_model_list(ipls_agg *h, int target, uint8_t *out, int64_t out_cap);

/* DownloadMapParameters plus what the Updater does with the map: for every p
 * of parts[0..n_parts) (the ChangedList; parts == NULL: every key of the file)
 *   mode IPLS_SAVED_SET:   target[p][i] = file[p][i]
 *   mode IPLS_SAVED_BLEND: target[p][i] = a*target[p][i] + b*file[p][i]
 *        (the leaving-peer blend, a = 0.6, b = 1 - 0.6; ipls_agg_blend's arithmetic)
 * for i < L_p.  A listed p that the file lacks is IPLS_E_RANGE (Java:
 * parameters.get(p) == null, then a NullPointerException in the Updater), so
 * is a file array shorter than L_p (ArrayIndexOutOfBounds, Updater.java:67)
 * and a key outside [0, P); a longer array contributes its first L_p values.
 * Everything is validated before the first launch: an error leaves every
 * target as it was.  The file goes to each GPU once; one launch per shard
 * decodes the payloads where they lie in it.  *applied (nullable) receives
 * the number of partitions written. */
int ipls_agg_load_saved(ipls_agg *h, const uint8_t *bytes, int64_t n, int mode, int target, const int32_t *parts,
                        int n_parts, double a, double b, int32_t *applied);

#ifdef __cplusplus
}
#endif
#endif /* IPLS_AGG_H */
