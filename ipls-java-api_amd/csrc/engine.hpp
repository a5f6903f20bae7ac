// engine.hpp -- the single-device aggregation engine (engine.hip) as the
// multi-device front (ipls_agg.cpp) sees it.  One engine holds the
// accumulators of a contiguous block of the handle's partitions on one GPU;
// engine partition q is handle partition p_lo + q.  Every function has the
// meaning of the C-ABI entry point of the same suffix (include/ipls_agg.h)
// restricted to that block; none of them is exported from the library.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/ipls_agg.h"
#include "fmt.hpp"

struct ipls_dev;
struct ipls_stage;   // the staging one chunked call owns (stage.hpp)

const char* dev_last_error(const ipls_dev* h);
void dev_set_thread_error(const char* msg);
// The calling thread's current HIP device, tracked while a C-ABI call runs so
// that switching to a device that is already current costs no HIP call:
// dev_use(d) makes d current (hipSetDevice only when the tracked device
// differs); dev_track(d) records what the thread's device is (-1: unknown,
// every dev_use then sets it); dev_tracked() returns the record.  Every device
// switch on a calling thread goes through dev_use, so the record stays exact.
hipError_t dev_use(int device);
void dev_track(int device);
int dev_tracked();
int dev_geometry(const ipls_agg_cfg* cfg, std::vector<int64_t>& len, std::vector<int64_t>& off, int64_t& chunk,
                 std::string& why);
int dev_open(const ipls_agg_cfg* cfg, int device, int p_lo, int p_hi, ipls_dev** out);
int dev_close(ipls_dev* h);
int dev_device(const ipls_dev* h);
void* dev_stream(ipls_dev* h);
int dev_sync(ipls_dev* h);
int dev_wait(ipls_dev* h, uint64_t ticket);
int dev_flush(ipls_dev* h);
int dev_set_coalesce(ipls_dev* h, int max_group);
int dev_last_launch(const ipls_dev* h, ipls_launch_info* out);

int dev_load_model(ipls_dev* h, const void* src, int64_t n, int src_kind);
int dev_split(ipls_dev* h, const void* flat, int64_t n, int src_kind, int p, void* dst, int dst_kind);
int dev_update_gradient(ipls_dev* h, const void* flat, int64_t n, int src_kind, const int32_t* owned, int n_owned);
int dev_accumulate(ipls_dev* h, int p, int target, const void* src, int64_t n, int src_kind);
int dev_accumulate_async(ipls_dev* h, int p, int target, const void* src, int64_t n, int src_kind, uint64_t* ticket);
int dev_accumulate_range(ipls_dev* h, int p, int target, const void* src, int64_t off, int64_t n, int src_kind,
                         uint64_t* ticket);
int dev_read_range(ipls_dev* h, int p, int target, void* dst, int64_t off, int64_t n, int dst_kind, uint64_t* ticket);
int dev_accumulate_chunked(ipls_dev* h, int p, int target, int64_t n, int src_kind, int64_t chunk,
                           ipls_chunk_source source, void* ctx);
int dev_accumulate_chunked_narrow(ipls_dev* h, int p, int target, int64_t n, int src_kind, int64_t chunk,
                                  ipls_chunk_source source, void* ctx);
// ---- ipls_agg_update_gradient_chunked: one stage per involved shard ----
// The front plans the call (flat_plan.hpp) and feeds the stages in flat order:
// dev_flat_begin (a stage whose device buffer holds `seg` elements of `fmt`
// plus padding, pinned slots of slot_elems), then per source call
// dev_flat_slot (the slot chunk k of THIS stage is received into, free to
// write) and dev_flat_copy (its H2D ranges, in elements: slot -> segment),
// dev_flat_landed after the stage's last chunk.  No engine lock is taken by
// any of them.  dev_flat_commit then applies every stage of the call as one
// unit (the engines' locks in the order given, all held at once; per shard
// flush_pending, a wait for its copies, its launches of k_update_flat) and
// releases the stages; a call that fails before it gives each stage back with
// dev_stage_release and its error.
struct flat_job {
  int q;                 // engine-local partition
  int64_t lo, ncopy;     // first element in the staged segment, values copied
};
struct flat_commit {
  ipls_dev* h;
  ipls_stage* st;
  const flat_job* jobs;      // the launches' jobs back to back
  const int* launch_len;     // jobs per launch (no partition twice in one)
  int n_launches;
};
int dev_flat_begin(ipls_dev* h, Fmt fmt, int64_t seg, int64_t slot_elems, ipls_stage** st);
int dev_flat_slot(ipls_dev* h, ipls_stage* st, int64_t k, void** host);
int dev_flat_copy(ipls_dev* h, ipls_stage* st, int64_t k, Fmt fmt, const int64_t* src, const int64_t* dst,
                  const int64_t* n, int n_copies);
int dev_flat_landed(ipls_dev* h, ipls_stage* st);
int dev_flat_commit(const flat_commit* c, int n, Fmt fmt);
int dev_finalize_chunked(ipls_dev* h, int p, int sum_kind, int64_t chunk, ipls_chunk_sink sink, void* ctx);
// the two phases of ipls_agg_get_partitions_chunked on one engine: the snapshot under the
// engine lock (into a stage the call owns; null for an empty segment), then
// the delivery to the sink with no lock held
// (fmt: a trainer format makes the snapshot the narrowed model, which
// dev_get_partitions_deliver_narrow hands out as bytes)
int dev_get_partitions_snapshot(ipls_dev* h, int64_t chunk, bool wire, ipls_stage** st, Fmt fmt = kFmtF64);
int dev_get_partitions_deliver(ipls_dev* h, ipls_stage* st, int64_t chunk, ipls_chunk_sink sink, void* ctx);
int dev_get_partitions_deliver_narrow(ipls_dev* h, ipls_stage* st, int64_t chunk, Fmt fmt, ipls_byte_sink sink,
                                      void* ctx);
// Stage ownership, one rule: a stage that dev_flat_begin, dev_get_partitions
// _snapshot or dev_ser_pack handed out stays the caller's through every
// dev_flat_* step and dev_*_deliver and goes back through exactly one
// dev_stage_release with the call's result (null st: nothing to do) -- but a
// dev_flat_commit takes its stages with it.  IPLS_OK returns the stage to the
// pool; anything else (a source or sink that stopped, a snapshot never
// delivered) first waits for its copies and its snapshot (the give-up path of
// stage.hpp's release).
void dev_stage_release(ipls_dev* h, ipls_stage* st, int rc);
int dev_update_indirect(ipls_dev* h, int p, int target, const void* bytes, int64_t n_bytes);
int dev_gbuf_load(ipls_dev* h, const void* bytes, int64_t n_bytes, const void** gbuf, int64_t* glen);
int dev_other_replica(ipls_dev* h, int p, int32_t aggregator, const void* src, int64_t n, int src_kind);
int dev_other_check(ipls_dev* h);
int dev_other_replica_drop(ipls_dev* h, int p, int32_t aggregator);
// order: n_order engine-local (p, aggregator) pairs, every stored key once
int dev_collect_replicas(ipls_dev* h, int32_t* participants, const int32_t* order, int n_order);
int dev_reduce_batch(ipls_dev* h, int p_first, int n_parts, const void* const* bufs, int k, int src_kind,
                     int start_mode, int target);
int dev_reduce_batch_out(ipls_dev* h, int p_first, int n_parts, const void* const* bufs, int k, int src_kind,
                         int start_mode, void* const* dst, int dst_kind);
int dev_reduce_ext(ipls_dev* h, int n, const int64_t* lens, const void* const* bufs, int k, bool be_in,
                   int start_mode, void* const* dst);
int dev_ingest_pubsub(ipls_dev* h, int target, const uint8_t* const* msgs, const int64_t* lens, int n_msgs,
                      int layers, const int32_t* parts, int32_t* status);
int dev_blend(ipls_dev* h, int p, int target, const void* src, int64_t n, int src_kind, double a, double b);
int dev_scale(ipls_dev* h, int p, int dst_target, int src_target, double c);
int dev_finalize(ipls_dev* h, int p, void* sum_out, int sum_kind, double* avg_out);
int dev_aggregate_round(ipls_dev* h, int p_first, int n_parts, const void* const* bufs, int k, int src_kind,
                        void* avg_out, int avg_kind);
int dev_set_weights(ipls_dev* h, int p, const void* src, int64_t n, int src_kind);
int dev_get_partitions(ipls_dev* h, void* out, int64_t n, int out_kind);
int dev_read(ipls_dev* h, int p, int target, void* dst, int64_t n, int dst_kind);
int dev_promote_future(ipls_dev* h, const int32_t* parts, int n_parts);
int dev_reset(ipls_dev* h, int p);
int dev_device_ptr(ipls_dev* h, int p, int target, void** ptr);
int dev_checksum(ipls_dev* h, int p, int target, uint64_t* out);
int64_t dev_commit_partial(ipls_dev* h, int p, int32_t workers, uint8_t* out, int64_t out_cap);
int64_t dev_merge_files(ipls_dev* h, const uint8_t* const* files, const int64_t* lens, int k, int file_kind,
                        uint8_t* out, int64_t out_cap);
int64_t dev_publish_many(ipls_dev* h, int n, const int* parts, int target, int32_t a, const int32_t* b, int16_t pid,
                         const uint8_t* origin, int32_t origin_len, void* out, const int64_t* offs,
                         const int64_t* lens, int out_kind);
int64_t dev_publish(ipls_dev* h, int p, int target, int32_t a, int32_t b, int16_t pid, const uint8_t* origin,
                    int32_t origin_len, void* out, int64_t out_cap, int out_kind);
// SendGradients: the pubsub texts of partitions parts[0..n_parts) (engine indices) of the flat vector, laid out
// by the front as for dev_publish_many.  flat == null: the n = 0 texts, encoded on the host.
int64_t dev_send_many(ipls_dev* h, const void* flat, int64_t n, int src_kind, int n_parts, const int* parts,
                      int32_t iteration, int16_t pid, const uint8_t* origin, int32_t origin_len, void* out,
                      const int64_t* offs, const int64_t* lens, int out_kind);

// ---- the segment-list calls (ipls_agg_*_segs; seg_plan.hpp, seg_kernels.hpp) ----
// The flat vector is the concatenation of n_segs device arrays.  The front has
// validated the table (kinds, alignment, lengths); the engine plans its own
// part -- the segments that meet its flat segment -- and launches once per
// repeat level (update), once (divide, send).  fmt: a segplan format code.
struct seg_ref {
  const void* ptr;
  int64_t n;
  int fmt;
};
int dev_update_gradient_segs(ipls_dev* h, const seg_ref* segs, int n_segs, const int32_t* owned, int n_owned);
int dev_get_partitions_segs(ipls_dev* h, const seg_ref* segs, int n_segs);
int64_t dev_send_many_segs(ipls_dev* h, const seg_ref* segs, int n_segs, int n_parts, const int* parts,
                           int32_t iteration, int16_t pid, const uint8_t* origin, int32_t origin_len, void* out,
                           const int64_t* offs, const int64_t* lens, int out_kind);

// The difference calls (ipls_agg_*_segs_diff; seg_diff_kernels.hpp): segs is the minuend list and makes the plan;
// b_ptrs[s] is the subtrahend array of segment s, of segs[s]'s length and format (not looked at when that is empty).
// They share the twins' code: a twin is the same path with no subtrahend list.
int dev_update_gradient_segs_diff(ipls_dev* h, const seg_ref* segs, const void* const* b_ptrs, int n_segs,
                                  const int32_t* owned, int n_owned);
int64_t dev_send_many_segs_diff(ipls_dev* h, const seg_ref* segs, const void* const* b_ptrs, int n_segs, int n_parts,
                                const int* parts, int32_t iteration, int16_t pid, const uint8_t* origin,
                                int32_t origin_len, void* out, const int64_t* offs, const int64_t* lens, int out_kind);

// The peer-list call (ipls_agg_update_gradient_segs_peers; seg_peers_kernels.hpp): n_peers lists over one table.
// segs makes the plan: the shared minuend list (diff), else peer 0's list.  t_ptrs[k * n_segs + s] is peer k's
// array of segment s, of segs[s]'s length and format (not looked at when that is empty).  One launch: a partition
// repeated in `owned` becomes a multiplicity of its job.
int dev_update_gradient_segs_peers(ipls_dev* h, const seg_ref* segs, bool diff, const void* const* t_ptrs, int n_peers,
                                   int n_segs, const int32_t* owned, int n_owned);

// The output-copy-list call (ipls_agg_get_partitions_segs_copies; seg_copies_kernels.hpp): n_lists lists over one
// table, every one written with the twin's bits.  segs is list 0 and makes the plan; o_ptrs[k * n_segs + s] is list
// k's array of segment s, of segs[s]'s length and format (not looked at when that is empty).  One launch.
int dev_get_partitions_segs_copies(ipls_dev* h, const seg_ref* segs, void* const* o_ptrs, int n_lists, int n_segs);

// The many-trainers round (ipls_agg_round_segs_peers; seg_round_kernels.hpp): the peer-list fold, W = AGG + REP and
// the output-copy-list divide of the engine's partitions in one launch.  segs, diff, t_ptrs and n_peers as for
// dev_update_gradient_segs_peers, o_ptrs and n_lists as for dev_get_partitions_segs_copies; `owned` lists the
// engine partitions that are folded and finalized (repeats are multiplicities), every other partition's W is read
// only.  An output list may be the minuend list or a peer list (same arrays).
int dev_round_segs_peers(ipls_dev* h, const seg_ref* segs, bool diff, const void* const* t_ptrs, int n_peers,
                         void* const* o_ptrs, int n_lists, int n_segs, const int32_t* owned, int n_owned);

// ---- saved-model files (javaser.hpp; ipls_agg_save_model* / _load_saved) ----
// One run of a file that an engine packs: `prefix` (framing), then engine
// partition q's values of `target`, then `suffix` (a byte, or -1).
struct ser_entry {
  int q;
  int32_t prefix_len, suffix;
  unsigned char prefix[192];
};
// Pack the entries back to back, in the order given, into a stage of the
// call's own (pinned slots of slot_bytes) under the engine lock: one launch.
// boxed: 14-byte Double records (DLIST) instead of a double[] payload.
// *nbytes is the image's length; hand it out with dev_ser_deliver, then
// dev_stage_release.
int dev_ser_pack(ipls_dev* h, const ser_entry* entries, int n, int target, bool boxed, int64_t slot_bytes,
                 ipls_stage** st, int64_t* nbytes);
// Image bytes [off, off + n) to the sink in pieces of at most `chunk`, as file
// bytes base, base + 1, ...; no lock held.
int dev_ser_deliver(ipls_dev* h, ipls_stage* st, int64_t off, int64_t n, int64_t chunk, int64_t base,
                    ipls_byte_sink sink, void* ctx);
// target[q[i]] = or blended with the big-endian payload at file byte offs[i]
// (validated by the caller: in range, at least L_q values): the file's bytes
// [lo, hi) go up once, one launch applies every entry.
int dev_ser_apply(ipls_dev* h, const uint8_t* bytes, int64_t lo, int64_t hi, const int* q, const int64_t* offs, int n,
                  int mode, int target, double a, double b);
// InitializeWeights from a DLIST whose header the caller has parsed (nvals
// elements): the engine decodes and checks records [flat_base, hi) on its GPU
// (hi < 0: to the end of its own segment),
// IPLS_E_FORMAT if one is not a Double; with `apply` it then loads its segment.
int dev_load_dlist(ipls_dev* h, const uint8_t* bytes, int64_t nvals, int64_t hi, bool apply);
