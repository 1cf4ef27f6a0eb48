/*
 * janus_prio3.h -- C ABI of the MI355X (gfx950) batched Prio3 helper prepare+aggregate
 * engine.  This is the drop-in boundary a Janus FFI crate binds.
 *
 * It replaces, for a whole aggregation-job batch in one device call:
 *   - the VDAF part of the helper's per-report loop in
 *     VdafOps::handle_aggregate_init_generic, /root/reference/aggregator/src/aggregator.rs:2020-2042
 *     (prio `helper_initialized(verify_key, agg_param, nonce, public_share, input_share,
 *      inbound)` followed by `PingPongTransition::evaluate`, i.e. prio 0.16.2 Prio3
 *      prepare_init(agg_id=1) -> decode leader PrepareShare ->
 *      prepare_shares_to_prepare_message([leader, helper]) -> prepare_next);
 *   - the per-report accumulate in AggregationJobWriter::
 *     update_batch_aggregations_from_report_aggregations,
 *     /root/reference/aggregator/src/aggregator/aggregation_job_writer.rs:591-695
 *     (BatchAggregation::merged_with -> AggregateShare::merge,
 *      /root/reference/aggregator_core/src/datastore/models.rs:1318-1372).
 * The instance it is created for corresponds to one arm of `vdaf_dispatch!`
 * (/root/reference/core/src/vdaf.rs:198-300): Prio3Count, Prio3Sum{bits},
 * Prio3SumVec{bits,length,chunk_length}, Prio3Histogram{length,chunk_length}.
 *
 * Conventions: plain pointers and sizes, caller-owned buffers, no callbacks.  All
 * per-report byte strings are fixed-length for a given instance (see prio3_sizes).
 * A per-report failure never aborts the batch; it is reported in status_out.
 */
#ifndef JANUS_PRIO3_H
#define JANUS_PRIO3_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* VDAF kinds (VdafInstance variants, core/src/vdaf.rs:65-108). */
enum {
  PRIO3_COUNT = 0,     /* Prio3::new_count(2)                         (vdaf.rs:201-208) */
  PRIO3_SUM = 1,       /* Prio3::new_sum(2, bits)                     (vdaf.rs:210-217) */
  PRIO3_SUMVEC = 2,    /* Prio3::new_sum_vec_multithreaded(2, ...)    (vdaf.rs:219-235) */
  PRIO3_HISTOGRAM = 3, /* Prio3::new_histogram(2, length, chunk)      (vdaf.rs:257-266) */
  /* Prio3SumVecField64MultiproofHmacSha256Aes128 (vdaf.rs:173-195, algorithm 0xFFFF1003):
   * SumVec<Field64, ParallelSum<Mul>> with XofHmacSha256Aes128, 32-byte seeds and verify key,
   * num_proofs >= 2.  Created with prio3_engine_create_ex (32-byte verify key); helper role. */
  PRIO3_SUMVEC_F64_MP = 4,
  /* Prio3FixedPointBoundedL2VecSum<FixedI16<U15> | FixedI32<U31>> (vdaf.rs:26-31, 292-335,
   * algorithm 0xFFFF0000): bits = 16 or 32 (the BitSize), length = entries; chunk_length is
   * ignored (both gadgets use optimal_chunk_length, as prio does).  Helper role.  The circuit
   * is reconstructed (prio's fixedpoint_l2.rs is not in the reference): DESIGN.md section 10. */
  PRIO3_FPVEC_BOUNDED_L2 = 5,
};

/* Per-report status; each maps 1:1 to the PingPongError variant prio returns and to the
 * metric label Janus records in handle_ping_pong_error
 * (/root/reference/aggregator/src/aggregator/error.rs:365-428). */
enum {
  PRIO3_STATUS_FINISHED = 0,          /* PingPongState::Finished + PingPongMessage::Finish */
  PRIO3_STATUS_PREP_INIT = 1,         /* VdafPrepareInit -> "prepare_init_failure" */
  PRIO3_STATUS_PREP_SHARE_DECODE = 2, /* CodecPrepShare -> "leader_prep_share_decode_failure" */
  PRIO3_STATUS_PREP_MSG = 3,          /* VdafPrepareSharesToPrepareMessage (decide failed) */
  PRIO3_STATUS_PREP_NEXT = 4,         /* VdafPrepareNext (joint randomness mismatch) */
  PRIO3_STATUS_PEER_MISMATCH = 5,     /* PeerMessageMismatch (set by the host framing layer) */
  PRIO3_STATUS_INPUT_SHARE_DECODE = 6, /* leader: input share not canonical -> PrepareError::
                                          InvalidMessage (aggregation_job_driver.rs:397-415) */
};

/* Merged per-report status of prio3_helper_aggregate_init_batch[_ex] for a report the helper
 * rejects before its VDAF runs: 0x80 | the DAP PrepareError Janus records (messages/src/lib.rs
 * PrepareError; aggregator.rs:1847-2015), which takes precedence over any VDAF status.  Among
 * themselves they take the order of aggregator.rs: the open and decode (0x84 / 0x88) first, then
 * the report deadline (0x89). */
enum {
  PRIO3_STATUS_HPKE_DECRYPT = 0x84,     /* PrepareError::HpkeDecryptError (open / AAD failed) */
  PRIO3_STATUS_INVALID_MESSAGE = 0x88,  /* PrepareError::InvalidMessage (PlaintextInputShare,
                                           extensions, helper input share length) */
  PRIO3_STATUS_REPORT_TOO_EARLY = 0x89, /* PrepareError::ReportTooEarly (time after the deadline) */
};

/* Whole-call return codes. */
enum {
  PRIO3_OK = 0,
  PRIO3_EINVAL = -1,   /* bad parameters / sizes */
  PRIO3_EDEVICE = -2,  /* HIP error (device lost, OOM): caller falls back to its CPU path */
  PRIO3_EUNSUPPORTED = -3,
};

typedef struct {
  uint32_t kind;         /* PRIO3_* */
  uint32_t bits;         /* Sum, SumVec; FPVec bit size (16 or 32) */
  uint32_t length;       /* SumVec, Histogram, FPVec entries */
  uint32_t chunk_length; /* SumVec, Histogram */
  uint32_t num_proofs;   /* 1 for every standard Prio3 instance */
} prio3_params;

typedef struct {
  uint32_t field_bytes;       /* 8 (Field64) or 16 (Field128) */
  uint32_t meas_len, out_len, proof_len, verifier_len, joint_rand_len;
  uint32_t nonce_len;         /* 16 (report ID) */
  uint32_t public_share_len;  /* 2 seeds with joint randomness (32 B; 64 B for 32-byte seeds) */
  uint32_t helper_share_len;  /* 3 seeds with joint randomness, else 2 (16- or 32-byte seeds) */
  uint32_t prep_share_len;    /* leader PrepareShare bytes (verifiers || jr part) */
  uint32_t prep_msg_len;      /* one seed with joint randomness (16 or 32 B), else 0 */
  uint32_t agg_share_len;     /* out_len * field_bytes */
  uint32_t leader_input_share_len; /* enc(meas share) || enc(proofs share) [|| k_blind] */
} prio3_sizes_t;

typedef struct prio3_engine prio3_engine;
typedef struct prio3_batch prio3_batch;

int prio3_sizes(const prio3_params* params, prio3_sizes_t* out);

/* Created where Janus builds VdafOps for a task (aggregator.rs:880-988): one engine per
 * (VDAF instance, verify key), bound to one GPU. */
int prio3_engine_create(const prio3_params* params, const uint8_t verify_key[16], int device,
                        prio3_engine** out);
/* As prio3_engine_create with a verify key of verify_key_len bytes: 16 for the TurboSHAKE
 * instances, 32 for PRIO3_SUMVEC_F64_MP (VERIFY_KEY_LENGTH_HMACSHA256_AES128, vdaf.rs). */
int prio3_engine_create_ex(const prio3_params* params, const uint8_t* verify_key,
                           size_t verify_key_len, int device, prio3_engine** out);
void prio3_engine_destroy(prio3_engine* engine);

/* One engine over several GPUs of the node: the `device_mask` form of SURVEY.md 8(b)'s
 * prio3_engine_create.  A Janus helper process that owns the node's GPUs creates each task's
 * engine over all of them (bit d = GPU d).  Host-buffer jobs (prio3_helper_prepare_batch,
 * prio3_helper_prepare_aggregate_batch, prio3_leader_prepare_init_batch) go whole to the GPU
 * whose executor holds the fewest reports -- the jobs of every engine of the same VDAF instance
 * counted, equally loaded GPUs taken in turn -- and are coalesced there with the other engines'
 * concurrent jobs.  No collective: a job's outputs (prepare messages, statuses, aggregate shares,
 * batch handle) come back whole from the GPU that ran it, and Janus already merges per-job
 * aggregations at collection (aggregation_job_writer.rs:510 writes a random `ord` shard per job;
 * aggregate_share.rs:55-96 sums them).  Device-resident entry points act on the lowest GPU of the
 * mask.  Options set on the engine apply to every GPU's part. */
int prio3_engine_create_mask(const prio3_params* params, const uint8_t* verify_key,
                             size_t verify_key_len, int device_mask, prio3_engine** out);
/* The same over an explicit device list; a GPU named k times gets k executors of its own (lanes
 * 0..k-1, at most 8), which lets a one-GPU box rehearse the placement (tests). */
int prio3_engine_create_devices(const prio3_params* params, const uint8_t* verify_key,
                                size_t verify_key_len, const int* devices, uint32_t n_devices,
                                prio3_engine** out);
typedef struct {
  int32_t device;        /* the member's GPU */
  uint32_t lane;         /* its executor on that GPU (0 unless the device list repeats the GPU) */
  uint64_t jobs;         /* host-buffer jobs this engine placed on the member */
  uint64_t reports;      /* their reports */
  uint64_t exec_jobs;    /* jobs the member's helper executor took (every engine sharing it) */
  uint64_t exec_groups;  /* group launches of that executor */
} prio3_member_info;
/* Fills out[0 .. min(cap, members)) and returns the member count (1 for a one-GPU engine). */
int prio3_engine_members(const prio3_engine* engine, prio3_member_info* out, uint32_t cap);
/* Counters of one executor a member's jobs use (shared with every engine of the same instance on
 * that GPU): kind 0 helper prepare, 1 accumulate, 2 leader prepare_init, 3 leader prepare_next,
 * 5 leader upload (4 is the HPKE open's, janus_hpke_executor_stats_get). */
typedef struct {
  uint64_t jobs, reports;  /* submitted since the process started */
  uint64_t groups;         /* launches */
  uint64_t active_jobs, active_reports;  /* inside the executor now */
} prio3_executor_stats;
int prio3_executor_stats_get(const prio3_engine* engine, uint32_t member, int kind,
                             prio3_executor_stats* out);
/* Executor control on the executors of `kind` (as above; -1: every kind) that the engine's jobs
 * use (shared with the other engines of the same GPUs): "hold" = 1 -- launch nothing until
 * "hold" = 0 (tests queue jobs behind it to pin coalescing); "heavy" = N -- reports inside the
 * executor at which it switches from its light-load pipeline to the heavy-load launcher
 * (0: the default 32768; 1: always the heavy-load one). */
int prio3_executor_control(prio3_engine* engine, int kind, const char* key, int64_t value);

/* ---- Host-buffer entry points (what the Rust FFI calls from inside rayon::spawn) ---- */

/* Prepares n reports.  Inputs are packed per report:
 *   nonces[n][16]  (report IDs), public_shares[n][public_share_len],
 *   helper_shares[n][helper_share_len], leader_prep_shares[n][prep_share_len]
 *   (the prep_share of each PingPongMessage::Initialize, framing already removed).
 * Outputs: prep_msgs_out[n][prep_msg_len] (the Finish message payload) and status_out[n].
 * The output shares stay on the device inside *batch_out until prio3_accumulate.
 * Thread-safe: concurrent calls (from any engines of the same VDAF instance on the same GPU,
 * whatever their verify keys) are coalesced by the GPU's executor into shared launches.
 * Each batch owns the device state of its own call: batches of one engine may be accumulated
 * in any order, also after later prepares (free each with prio3_batch_free).
 * PRIO3_FPVEC_BOUNDED_L2 returns PRIO3_EUNSUPPORTED unless option "experimental_fpvec" is 1
 * (its circuit is a reconstruction; parity with prio unpinned). */
int prio3_helper_prepare_batch(prio3_engine* engine, uint32_t n, const uint8_t* nonces,
                               const uint8_t* public_shares, const uint8_t* helper_shares,
                               const uint8_t* leader_prep_shares, uint8_t* prep_msgs_out,
                               uint8_t* status_out, prio3_batch** batch_out);

/* Accumulates the finished reports whose accept_mask byte is non-zero (NULL = all) into
 * per-segment aggregate shares (segment = batch identifier, query_type.rs:72-82).  A segment id
 * >= n_segments excludes the report from every aggregate and count (all accumulate paths).
 * segment_ids (NULL = all segment 0) and accept_mask, when given, must each hold exactly n
 * entries (n = the batch's report count); n_segments >= 1.
 * agg_shares_out[n_segments][agg_share_len] (LE field elements, mod-p sums), counts_out. */
int prio3_accumulate(prio3_batch* batch, const uint32_t* segment_ids, const uint8_t* accept_mask,
                     uint32_t n_segments, uint8_t* agg_shares_out, uint64_t* counts_out);

/* prio3_helper_prepare_batch followed by prio3_accumulate of the same reports, in ONE coalesced
 * launch: the job's reports are accumulated into its n_segments aggregations in the group
 * launch that prepares them (no batch handle, no second round trip through the executor).
 * For callers whose accept mask is known before preparation (the host-side exclusions of the
 * aggregation job writer, aggregation_job_writer.rs:591-695); the output shares are not kept.
 * Same arguments and results as the two calls. */
int prio3_helper_prepare_aggregate_batch(prio3_engine* engine, uint32_t n, const uint8_t* nonces,
                                         const uint8_t* public_shares,
                                         const uint8_t* helper_shares,
                                         const uint8_t* leader_prep_shares,
                                         const uint32_t* segment_ids, const uint8_t* accept_mask,
                                         uint32_t n_segments, uint8_t* prep_msgs_out,
                                         uint8_t* status_out, uint8_t* agg_shares_out,
                                         uint64_t* counts_out);

/* The helper's whole per-report loop body for one aggregation job, from the sealed input shares
 * (VdafOps::handle_aggregate_init_generic, /root/reference/aggregator/src/aggregator.rs:1794-2096):
 * hpke::open of each report's encrypted input share (:1847-1890, the opener of janus_hpke.h, AAD
 * InputShareAad{task_id, metadata, public_share}), PlaintextInputShare decode and the extension
 * checks (:1893-1983; require_taskprov as in janus_hpke_open_input_shares), then
 * helper_initialized + evaluate (:2020-2042) and the accumulate of prio3_helper_prepare_aggregate_
 * batch -- in ONE coalesced group launch: concurrent jobs of every task of the instance that open
 * with the same keypair, ciphertext stride and taskprov flag share it, and the decrypted helper
 * shares never leave the GPU.  Inputs per report: report_ids[n][16] (the VDAF nonces), times[n]
 * (seconds), public_shares[n][public_share_len], enc[n][Nenc], ct[n][ct_stride] with ct_len[n],
 * leader_prep_shares[n][prep_share_len]; segment_ids / accept_mask / n_segments as in
 * prio3_accumulate.  status_out[n]: PRIO3_STATUS_* of the report's VDAF, or
 * PRIO3_STATUS_HPKE_DECRYPT / PRIO3_STATUS_INVALID_MESSAGE when the open rejected it (such a
 * report is never counted).  Instances whose public share is neither 0 nor 32 bytes
 * (PRIO3_SUMVEC_F64_MP) return PRIO3_EUNSUPPORTED here; the _ex form below takes them.  The opener
 * may be bound to any GPU: the open runs on the GPU the job is placed on.
 * This is prio3_helper_aggregate_init_batch_ex without a fallback keypair and without a report
 * deadline. */
struct janus_hpke_opener;
int prio3_helper_aggregate_init_batch(
    prio3_engine* engine, struct janus_hpke_opener* opener, uint32_t n,
    const uint8_t task_id[32], int require_taskprov, const uint8_t* report_ids,
    const uint64_t* times, const uint8_t* public_shares, const uint8_t* enc, const uint8_t* ct,
    const uint32_t* ct_len, uint32_t ct_stride, const uint8_t* leader_prep_shares,
    const uint32_t* segment_ids, const uint8_t* accept_mask, uint32_t n_segments,
    uint8_t* prep_msgs_out, uint8_t* status_out, uint8_t* agg_shares_out, uint64_t* counts_out);

/* The same call with the whole status contract of the loop body, still ONE coalesced group launch
 * (jobs also share it only with jobs of the same fallback keypair, or likewise none):
 *  - opener is the keypair tried first: the task's keypair for the reports' config id, or the
 *    global one when the task has none.  fallback_opener (NULL: none) is the global keypair when
 *    both exist (aggregator.rs:1864-1878): a report whose open under `opener` ends in
 *    HpkeDecryptError -- and only such a report; one that opened and then failed its decode or
 *    extension checks keeps 0x88 -- is opened again under fallback_opener inside the launch, and
 *    that plaintext passes the same decode and checks (so it ends in 0, 0x84 or 0x88).  Both
 *    openers must be of the same KEM (one enc[n][Nenc] layout), else PRIO3_EINVAL; a NULL opener is
 *    PRIO3_EINVAL.  A config id no keypair is known for (HpkeUnknownConfigId) stays with the
 *    caller: no keypair, no call.
 *  - report_deadline (seconds; UINT64_MAX: no check): a report with times[i] > report_deadline gets
 *    PRIO3_STATUS_REPORT_TOO_EARLY (aggregator.rs:2004-2015; a time equal to the deadline passes).
 *    Precedence: PRIO3_STATUS_HPKE_DECRYPT / _INVALID_MESSAGE, then _REPORT_TOO_EARLY, then the
 *    VDAF status.  Such a report is never counted and its prepare message is undefined, as for
 *    the open's rejections.  Concurrent jobs of one task may carry different deadlines.
 *  - every instance is admitted, PRIO3_SUMVEC_F64_MP included (64-byte public shares, 96-byte
 *    helper shares, 32-byte prepare messages). */
int prio3_helper_aggregate_init_batch_ex(
    prio3_engine* engine, struct janus_hpke_opener* opener,
    struct janus_hpke_opener* fallback_opener, uint64_t report_deadline, uint32_t n,
    const uint8_t task_id[32], int require_taskprov, const uint8_t* report_ids,
    const uint64_t* times, const uint8_t* public_shares, const uint8_t* enc, const uint8_t* ct,
    const uint32_t* ct_len, uint32_t ct_stride, const uint8_t* leader_prep_shares,
    const uint32_t* segment_ids, const uint8_t* accept_mask, uint32_t n_segments,
    uint8_t* prep_msgs_out, uint8_t* status_out, uint8_t* agg_shares_out, uint64_t* counts_out);

/* ---- One-call helper job ---- */
/* A whole helper aggregation job as AggregationJobWriter needs it (aggregation_job_writer.rs:
 * 540-695, aggregator.rs:1765-1773), in ONE trip through the executor: the job index
 * (prio3_job_index below: batch-identifier index, BatchCollected rejections, duplicate-ID verdict),
 * the loop body of prio3_helper_aggregate_init_batch_ex, and the per-batch ReportIdChecksum and
 * client-timestamp interval of prio3_batch_metadata.  The result is byte for byte what this
 * composition of the three calls gives, and every rule of their sections holds unchanged:
 *   prio3_job_index(report_ids, times, time_precision, closed_intervals, k, max_segments, ...);
 *   accept[i] = the job index's accept byte AND accept_mask[i] != 0 (NULL mask: all ones);
 *   prio3_helper_aggregate_init_batch_ex(..., segment_ids, accept, n_segments = max_segments, ...);
 *   prio3_batch_metadata(report_ids, times, status, accept, segment_ids, max_segments, ...).
 * So the aggregate, count, checksum and interval rows are sized for max_segments segments (rows
 * >= info->n_segments: zero, count 0, Interval::EMPTY); at overflow every segment id is 0xFFFFFFFF
 * and nothing is counted while statuses and prepare messages stay valid; a duplicate ID marks a
 * report and rejects nothing; a report the host mask, a closed batch or its status excludes is in
 * no aggregate, count or checksum but still widens its batch's interval.  accept_mask (nullable)
 * carries the datastore's replay survivors, which stay the host's.
 * A job of at most PRIO3_JOB_GROUP_MAX_REPORTS reports and PRIO3_JOB_GROUP_MAX_SEGMENTS segments
 * (and max_segments aggregate shares within one group's staging) is indexed by one workgroup in
 * front of the coalesced group launch that opens, prepares and accumulates it, and its metadata
 * rows are made behind that accumulate; jobs that carry an index request share launches with each
 * other.  A larger job runs the three calls from inside this one -- no size is refused.
 * out->segment_starts, reject, duplicate, checksums and intervals may each be NULL (prep_msgs too
 * for an instance without joint randomness); closed_intervals is read before the call returns.
 * Errors: those of the three calls (PRIO3_EINVAL for max_segments 0 or above 4096, k > 1024,
 * n > 2^30, a missing buffer). */
enum { PRIO3_JOB_GROUP_MAX_REPORTS = 4096, PRIO3_JOB_GROUP_MAX_SEGMENTS = 64 };
typedef struct {            /* what the job index found (section "Job index" below) */
  uint32_t n_segments;      /* distinct batch identifiers found, if <= max_segments */
  uint32_t overflow;        /* 1: more than max_segments distinct identifiers */
  uint32_t n_duplicates;    /* reports whose ID also occurs at a lower index */
  uint32_t first_duplicate; /* lowest such index; 0xFFFFFFFF if none */
  uint32_t n_closed;        /* reports in a closed batch */
  uint32_t n_time_errors;   /* reports whose batch interval overflows u64 */
} prio3_job_index_info;
typedef struct {
  struct janus_hpke_opener* opener;          /* as prio3_helper_aggregate_init_batch_ex */
  struct janus_hpke_opener* fallback_opener; /* nullable */
  uint64_t report_deadline;                  /* UINT64_MAX: no check */
  uint32_t n;
  int32_t require_taskprov;
  const uint8_t* task_id;                    /* [32] */
  const uint8_t* report_ids;                 /* [n][16] */
  const uint64_t* times;                     /* [n] */
  const uint8_t* public_shares;              /* [n][public_share_len] */
  const uint8_t* enc;                        /* [n][Nenc] */
  const uint8_t* ct;                         /* [n][ct_stride] */
  const uint32_t* ct_len;                    /* [n] */
  const uint8_t* leader_prep_shares;         /* [n][prep_share_len] */
  uint32_t ct_stride;
  uint32_t k;                                /* closed intervals */
  uint64_t time_precision;                   /* 0: a fixed-size task */
  const uint64_t* closed_intervals;          /* host [k][2] (start, duration); NULL when k = 0 */
  const uint8_t* accept_mask;                /* host [n], nullable */
  uint32_t max_segments;
  uint32_t reserved;                         /* 0 */
} prio3_helper_job_in;
typedef struct {
  uint32_t* segment_ids;                     /* [n] */
  uint64_t* segment_starts;                  /* [max_segments], nullable */
  uint8_t* reject;                           /* [n], nullable */
  uint8_t* duplicate;                        /* [n], nullable */
  prio3_job_index_info* info;
  uint8_t* prep_msgs;                        /* [n][prep_msg_len] */
  uint8_t* status;                           /* [n] */
  uint8_t* agg_shares;                       /* [max_segments][agg_share_len] */
  uint64_t* counts;                          /* [max_segments] */
  uint8_t* checksums;                        /* [max_segments][32], nullable */
  uint64_t* intervals;                       /* [max_segments][2], nullable */
} prio3_helper_job_out;
int prio3_helper_aggregate_job(prio3_engine* engine, const prio3_helper_job_in* job,
                               const prio3_helper_job_out* out);

/* Parity-only: copies the n output shares (n x agg_share_len). */
int prio3_debug_output_shares(prio3_batch* batch, uint8_t* out);
void prio3_batch_free(prio3_batch* batch);

/* ---- Device-resident entry points (buffers already in HBM; stream-ordered) ---- */
/* d_* are device pointers with the same packed layouts; stream is a hipStream_t, ordered like
 * any HIP call on it (NULL = the null stream, as in HIP itself -- so a caller whose inputs were
 * produced on the null stream needs no extra synchronisation).  The output shares of the
 * latest device-resident prepare of an engine stay on the device (its "current run") until the
 * next device-resident prepare of that engine replaces it; the accumulate / finish / output-share
 * calls act on that run. */
int prio3_device_prepare(prio3_engine* engine, uint32_t n, const uint8_t* d_nonces,
                         const uint8_t* d_public_shares, const uint8_t* d_helper_shares,
                         const uint8_t* d_leader_prep_shares, uint8_t* d_prep_msgs,
                         uint8_t* d_status, void* stream);
int prio3_device_accumulate(prio3_engine* engine, uint32_t n, const uint8_t* d_status,
                            const uint32_t* d_segment_ids, const uint8_t* d_accept_mask,
                            uint32_t n_segments, uint8_t* d_agg_shares, uint64_t* d_counts,
                            void* stream);
/* Prepare + aggregate in one pass.  Same as prio3_device_prepare, and additionally the output
 * shares of the batch are summed per segment (d_segment_ids[n], NULL = all in segment 0;
 * segment = batch identifier) while the measurement shares stream through the device
 * (Histogram: fused into the joint-randomness kernel; other instances: deferred to the
 * finish call).  prio3_device_aggregate_finish then applies the verdicts in d_status and
 * the host's accept mask (reports Janus drops after preparation -- replays, collected
 * batches: aggregation_job_writer.rs:540-588) and writes d_agg_shares[n_segments][agg_len]
 * and d_counts[n_segments].  Equivalent to prio3_device_prepare + prio3_device_accumulate. */
int prio3_device_prepare_aggregate(prio3_engine* engine, uint32_t n, const uint8_t* d_nonces,
                                   const uint8_t* d_public_shares, const uint8_t* d_helper_shares,
                                   const uint8_t* d_leader_prep_shares,
                                   const uint32_t* d_segment_ids, uint32_t n_segments,
                                   uint8_t* d_prep_msgs, uint8_t* d_status, void* stream);
int prio3_device_aggregate_finish(prio3_engine* engine, const uint8_t* d_status,
                                  const uint8_t* d_accept_mask, uint8_t* d_agg_shares,
                                  uint64_t* d_counts, void* stream);
/* The rest of the per-segment BatchAggregation update (aggregation_job_writer.rs:637-690,
 * models.rs:1318-1372), for the same batch and verdicts:
 *   d_checksums[n_segments][32]  ReportIdChecksum = XOR of SHA-256(report_id) over the reports
 *                                counted in d_counts (status FINISHED and accept mask non-zero;
 *                                core/src/report_id.rs:18-42);
 *   d_intervals[n_segments][2]   client-timestamp interval (start, duration) in seconds over
 *                                every report of the segment, failed ones included
 *                                (Interval::from_time + merge, core/src/time.rs:294-317);
 *                                (0, 0) = Interval::EMPTY for a segment without reports.
 * d_report_ids[n][16] are the report IDs (the VDAF nonces), d_times[n] the report timestamps
 * (NULL: intervals not computed).  Either output may be NULL.  Both are overwritten; merging
 * them into the batch aggregation already stored (XOR / Interval::merge) is the caller's. */
int prio3_device_batch_metadata(prio3_engine* engine, uint32_t n, const uint8_t* d_report_ids,
                                const uint64_t* d_times, const uint8_t* d_status,
                                const uint8_t* d_accept_mask, const uint32_t* d_segment_ids,
                                uint32_t n_segments, uint8_t* d_checksums, uint64_t* d_intervals,
                                void* stream);
/* Multi-GPU combine of k ranks' metadata after an all-gather: d_checksums_in[k][n_segments][32]
 * XORed, d_intervals_in[k][n_segments][2] merged (Interval::merge, empty = identity). */
int prio3_device_combine_metadata(prio3_engine* engine, uint32_t k, uint32_t n_segments,
                                  const uint8_t* d_checksums_in, const uint64_t* d_intervals_in,
                                  uint8_t* d_checksums_out, uint64_t* d_intervals_out,
                                  void* stream);
/* Host-buffer form of prio3_device_batch_metadata (blocking). */
int prio3_batch_metadata(prio3_engine* engine, uint32_t n, const uint8_t* report_ids,
                         const uint64_t* times, const uint8_t* status, const uint8_t* accept_mask,
                         const uint32_t* segment_ids, uint32_t n_segments, uint8_t* checksums_out,
                         uint64_t* intervals_out);
/* ---- Job index ---- */
/* The per-report bookkeeping that tells the accumulate which report goes where and which reports
 * may be counted, from the d_report_ids[n][16] and d_times[n] that janus_dap_agg_init_unpack_device
 * and prio3_device_leader_upload write, to the d_segment_ids / d_accept_mask the prepare, finish,
 * accumulate and metadata calls above read:
 *  - Batch identifier (TimeInterval::to_batch_identifier, aggregator_core/src/query_type.rs:72-82;
 *    Time::to_batch_interval_start, core/src/time.rs:207-224): start = t - t % time_precision.
 *    Segment s is the s-th distinct start in ASCENDING order (what numpy.unique(...,
 *    return_inverse=True) gives; the writer's by_batch_identifier_index,
 *    aggregation_job_writer.rs:598), written to d_segment_starts[s]; rows >= n_segments are zero.
 *    A report whose start + time_precision overflows a u64 (Interval::new fails) takes no segment:
 *    d_segment_ids = 0xFFFFFFFF, d_accept_mask = 0, counted in n_time_errors.
 *    time_precision == 0 is a fixed-size task: every report is in segment 0, n_segments = 1 when
 *    n > 0, d_segment_starts is not written and the closed intervals are not read.
 *  - Overflow: more than max_segments (1..4096) distinct starts give overflow = 1 and n_segments =
 *    max_segments + 1; the caller discards the job's other outputs.  They stay safe for the calls
 *    queued behind this one: every d_segment_ids[i] is then 0xFFFFFFFF with d_accept_mask[i] = 0
 *    and d_reject[i] = 0, d_segment_starts is zero and n_closed is 0 (n_time_errors, d_duplicate and
 *    the duplicate counts are what they are without overflow).  A caller that does not synchronise
 *    passes max_segments as n_segments to the later calls: empty segments come back with count 0,
 *    checksum 0 and Interval::EMPTY.
 *  - Closed batches (fail_report_aggregations_for_collected_batches, aggregation_job_writer.rs:
 *    540-588): closed_intervals is a HOST array [k][2] = (start, duration), k <= 1024 (NULL when
 *    k = 0), read before the call returns.  A segment is closed when its start lies in
 *    [start_j, start_j + duration_j) for some j (no wrap-around: an end past 2^64 - 1 closes
 *    every later start); the decision is made once per segment.  Its reports get d_accept_mask = 0
 *    and d_reject = PRIO3_REJECT_BATCH_COLLECTED (0x80 | PrepareError::BatchCollected, the
 *    convention of prio3_helper_aggregate_init_batch) and are counted in n_closed; every other
 *    report with a segment gets d_accept_mask = 1, and d_reject = 0 in any case.
 *  - Duplicate report IDs (the HashSet over every PrepareInit, aggregator.rs:1765-1773):
 *    d_duplicate[i] = 1 exactly when some j < i has the same 16 bytes (copies at 3, 7 and 9 mark 7
 *    and 9; first_duplicate = 7).  Nothing is rejected for it -- the reference fails the whole
 *    request, which stays the caller's decision -- and d_accept_mask does not depend on it.
 * Two runs over the same inputs give byte-identical outputs.  d_segment_starts, d_reject and
 * d_duplicate may each be NULL.  n == 0 succeeds with an all-zero info except first_duplicate.
 * PRIO3_EINVAL: n > 2^30, max_segments 0 or above 4096, k > 1024, a missing buffer.
 * Device form: stream-ordered, no host synchronisation, scratch from the GPU's pool (8 n to 16 n
 * bytes for the ID table); d_report_ids 16-byte aligned.  Host form: a plain blocking call. */
enum { PRIO3_REJECT_BATCH_COLLECTED = 0x80 };
/* prio3_job_index_info: declared above, ahead of prio3_helper_aggregate_job */
int prio3_device_job_index(prio3_engine* engine, uint32_t n, const uint8_t* d_report_ids,
                           const uint64_t* d_times, uint64_t time_precision,
                           const uint64_t* closed_intervals, uint32_t k, uint32_t max_segments,
                           uint32_t* d_segment_ids, uint64_t* d_segment_starts,
                           uint8_t* d_accept_mask, uint8_t* d_reject, uint8_t* d_duplicate,
                           prio3_job_index_info* d_info, void* stream);
int prio3_job_index(prio3_engine* engine, uint32_t n, const uint8_t* report_ids,
                    const uint64_t* times, uint64_t time_precision,
                    const uint64_t* closed_intervals, uint32_t k, uint32_t max_segments,
                    uint32_t* segment_ids, uint64_t* segment_starts, uint8_t* accept_mask,
                    uint8_t* reject, uint8_t* duplicate, prio3_job_index_info* info);

/* Copies the output shares of the last device prepare (n x agg_share_len) to host. */
int prio3_device_output_shares(prio3_engine* engine, uint32_t n, uint8_t* out);

/* Mod-p element-wise sum of k partial aggregate shares (the multi-GPU combine after an
 * RCCL all-gather; RCCL's integer sum is mod 2^64, not mod p).  d_in[k][n_segments*agg_len],
 * d_counts_in[k][n_segments] -> d_out[n_segments*agg_len], d_counts_out[n_segments]. */
int prio3_device_combine(prio3_engine* engine, uint32_t k, uint32_t n_segments,
                         const uint8_t* d_in, const uint64_t* d_counts_in, uint8_t* d_out,
                         uint64_t* d_counts_out, void* stream);

/* ---- Leader side ---- */
/* The leader's half of the same VDAF on the same engine: prio Prio3::prepare_init with
 * agg_id 0 on the explicit leader input shares (what PingPongTopology::leader_initialized
 * runs for each report in AggregationJobDriver::step_aggregation_job_aggregate_init,
 * /root/reference/aggregator/src/aggregator/aggregation_job_driver.rs:397-415), producing the
 * leader prepare shares that go into PingPongMessage::Initialize; then prepare_next on the
 * helper's prepare messages (leader_continued in process_response_from_helper, :677-691):
 * status becomes PREP_NEXT when the message is not the leader's joint-rand seed, and the
 * output shares stay on the device for prio3_accumulate / prio3_device_accumulate.
 * leader_input_shares[n][leader_input_share_len]; prep_shares_out[n][prep_share_len]. */
int prio3_leader_prepare_init_batch(prio3_engine* engine, uint32_t n, const uint8_t* nonces,
                                    const uint8_t* public_shares,
                                    const uint8_t* leader_input_shares, uint8_t* prep_shares_out,
                                    uint8_t* status_out, prio3_batch** batch_out);
int prio3_leader_prepare_next_batch(prio3_batch* batch, const uint8_t* prep_msgs,
                                    uint8_t* status_inout);
/* prio3_leader_prepare_next_batch followed by prio3_accumulate of the same batch, in ONE launch of
 * the GPU's prepare_next executor (concurrent jobs' checks and merges together): for a leader that
 * knows the job's batch identifiers and accept mask when the helper's response arrives
 * (process_response_from_helper, aggregation_job_driver.rs:629-691, then the writer's merge,
 * aggregation_job_writer.rs:591-695).  Same arguments and results as the two calls; the batch
 * keeps its output shares (it may be accumulated again) until prio3_batch_free. */
int prio3_leader_prepare_next_aggregate_batch(prio3_batch* batch, const uint8_t* prep_msgs,
                                              uint8_t* status_inout, const uint32_t* segment_ids,
                                              const uint8_t* accept_mask, uint32_t n_segments,
                                              uint8_t* agg_shares_out, uint64_t* counts_out);
/* ---- One-call leader job ---- */
/* What AggregationJobWriter needs from a leader job once the helper's response is decoded
 * (aggregation_job_driver.rs:629-770, aggregation_job_writer.rs:540-695), in ONE trip through the
 * prepare_next executor; n is the batch's.  The result is byte for byte this composition, and
 * every rule of the three calls' sections holds unchanged:
 *   status[i] = leader_status[i] if it is non-zero, else PRIO3_STATUS_PEER_MISMATCH (5) when
 *     prepare_error[i] != 0xFF, else 0 (prepare_error NULL: all 0xFF);
 *   prio3_job_index(report_ids, times, time_precision, closed_intervals, k, max_segments, ...);
 *   accept[i] = the job index's accept byte AND accept_mask[i] != 0 (NULL mask: all ones);
 *   prio3_leader_prepare_next_aggregate_batch(batch, prep_msgs, status, segment_ids, accept,
 *     max_segments, ...);
 *   prio3_batch_metadata(report_ids, times, status, accept, segment_ids, max_segments, ...);
 *   outcome[i] = 5 (VdafPrepError) if leader_status[i] != 0, else prepare_error[i] unless that is
 *     0xFF, else 5 if status[i] != 0, else 0 (BatchCollected) if reject[i] is set, else 0xFF
 *     (finished) -- a report that already failed keeps its error
 *     (aggregation_job_writer.rs:577-584).
 * So rows >= info->n_segments are zero, count 0, Interval::EMPTY; at overflow every segment id is
 * 0xFFFFFFFF and nothing is counted while statuses stay valid; a duplicate ID marks a report and
 * rejects nothing; an excluded report still widens its batch's interval; the batch keeps its
 * output shares (prio3_accumulate over segment_ids and the same accept bytes gives the same
 * aggregates afterwards).
 * A job of at most PRIO3_JOB_GROUP_MAX_REPORTS reports and PRIO3_JOB_GROUP_MAX_SEGMENTS segments
 * on a coalescable engine is indexed by one workgroup in front of the coalesced prepare_next
 * launch, accumulated behind it and its metadata rows made behind that; such jobs share launches
 * with each other.  Every other job (empty, larger, FPVec, the multiproof instance, coalesce off)
 * runs the composition from inside this call -- no size or instance is refused.
 * The helper's response is decoded in front of the call (janus_dap_agg_job_resp_unpack_host on the
 * caller's thread); the device decode is not part of it.
 * out->segment_starts, reject, duplicate, checksums, intervals and outcome may each be NULL;
 * closed_intervals is read before the call returns.
 * Errors: those of the three calls (PRIO3_EINVAL for max_segments 0 or above 4096, k > 1024, a
 * missing buffer), checked before anything is launched. */
typedef struct {
  const uint8_t* report_ids;                 /* [n][16] */
  const uint64_t* times;                     /* [n] */
  const uint8_t* leader_status;              /* [n]: what prio3_leader_prepare_init_batch wrote */
  const uint8_t* prepare_error;              /* [n]: what janus_dap_agg_job_resp_unpack_host wrote
                                                (0xFF = continued); NULL = all 0xFF */
  const uint8_t* prep_msgs;                  /* [n][prep_msg_len]; NULL without joint randomness */
  uint64_t time_precision;                   /* 0: a fixed-size task */
  const uint64_t* closed_intervals;          /* host [k][2] (start, duration); NULL when k = 0 */
  const uint8_t* accept_mask;                /* host [n], nullable: the replay survivors */
  uint32_t k;                                /* closed intervals */
  uint32_t max_segments;
} prio3_leader_job_in;
typedef struct {
  uint32_t* segment_ids;                     /* [n] */
  uint64_t* segment_starts;                  /* [max_segments], nullable */
  uint8_t* reject;                           /* [n], nullable */
  uint8_t* duplicate;                        /* [n], nullable */
  prio3_job_index_info* info;
  uint8_t* status;                           /* [n] merged leader status after prepare_next */
  uint8_t* outcome;                          /* [n], nullable: 0xFF finished, else the DAP
                                                PrepareError */
  uint8_t* agg_shares;                       /* [max_segments][agg_share_len] */
  uint64_t* counts;                          /* [max_segments] */
  uint8_t* checksums;                        /* [max_segments][32], nullable */
  uint64_t* intervals;                       /* [max_segments][2], nullable */
} prio3_leader_job_out;
int prio3_leader_finish_job(prio3_batch* batch, const prio3_leader_job_in* job,
                            const prio3_leader_job_out* out);
int prio3_device_leader_prepare_init(prio3_engine* engine, uint32_t n, const uint8_t* d_nonces,
                                     const uint8_t* d_public_shares,
                                     const uint8_t* d_leader_input_shares, uint8_t* d_prep_shares,
                                     uint8_t* d_status, void* stream);
int prio3_device_leader_prepare_next(prio3_engine* engine, uint32_t n, const uint8_t* d_prep_msgs,
                                     uint8_t* d_status, void* stream);
/* The device leader's output shares are summed by prio3_device_accumulate.  For Histogram the
 * sum is started inside prio3_device_leader_prepare_init (wave partials while the explicit
 * shares are unpacked; option leader_fuse_acc, default 1): an accumulate over the whole batch
 * with n_segments == 1 finishes from them (the verdicts, the accept mask and out-of-range
 * segment ids are applied as corrections), any other accumulate reads the output shares. */

/* ---- Ticketed job submission ---- */
/* Every job call above parks its caller for the whole device round trip, so a process has no more
 * jobs in flight than threads inside the library.  Each executor-backed job call has a submit
 * form: the same arguments as its blocking twin, plus notify_fd and ticket_out.  Submit stages the
 * job into its coalesced group on the calling thread and returns a ticket; prio3_ticket_wait
 * later blocks until the job's group has run, writes the outputs and returns what the blocking
 * call would have returned.  A thread may hold any number of tickets (Janus holds a rayon worker
 * only for CPU work and awaits a oneshot, aggregator.rs:2100-2123,
 * aggregation_job_driver.rs:449-462).
 *  - Inputs are read only inside the submit call -- every input array, closed_intervals, the
 *    accept mask, the task ID and the job structs themselves: the caller may reuse or free them as
 *    soon as submit returns.
 *  - Outputs are written only inside prio3_ticket_wait, on the waiting thread, and nothing is
 *    written after it returns.  Two exceptions: out->status of prio3_leader_finish_job_submit is
 *    in/out and is seeded (with leader_status) at submit; and the synchronous paths below write
 *    during submit.  The output buffers (and *batch_out of the leader's prepare_init) must stay
 *    valid until the wait.
 *  - notify_fd (-1: none) is a caller-owned eventfd; several tickets may share one.  Once the
 *    ticket's group is done -- with success or failure -- the library writes the 8-byte value 1 to
 *    it: exactly once per ticket, never before prio3_ticket_poll would return 1, and never from
 *    inside submit except on the synchronous paths.
 *  - Synchronous paths.  A job its blocking twin does not run as one executor job -- an empty
 *    job; one above PRIO3_JOB_GROUP_MAX_REPORTS / _MAX_SEGMENTS; an engine that cannot coalesce; a
 *    job with more segments than one group holds; a leader engine that is not coalescable (FPVec,
 *    the multiproof instance) -- runs that twin inside submit: the outputs are written there, the
 *    ticket comes back done, notify_fd is written before submit returns, and the wait returns the
 *    twin's result.  No size or instance is refused that the blocking form accepts;
 *    PRIO3_FPVEC_BOUNDED_L2 stays PRIO3_EUNSUPPORTED under the same rule.
 *  - Failure.  An argument error (or any failure before the job is queued) is the return value of
 *    submit, with *ticket_out = NULL: nothing is outstanding and notify_fd is not written.  A
 *    failure of the job's group is the return value of the wait.  A NULL ticket_out is
 *    PRIO3_EINVAL.
 *  - Ownership.  Every ticket must be waited exactly once, by one thread at a time; there is no
 *    cancel.  A ticket that is done but not yet waited keeps its group's pinned staging (96 MB per
 *    group) and counts as an active job of its executor until the wait.  Destroying an engine, an
 *    opener or a prio3_batch with tickets pending on it is a caller error, as destroying one under
 *    a blocked call is.
 *  - Coalescing.  Tickets of one thread share groups with each other and with blocking callers.
 *  - The calling thread's HIP device is left as it was, in submit and in wait. */
typedef struct prio3_ticket prio3_ticket;
int prio3_helper_prepare_aggregate_batch_submit(
    prio3_engine* engine, uint32_t n, const uint8_t* nonces, const uint8_t* public_shares,
    const uint8_t* helper_shares, const uint8_t* leader_prep_shares, const uint32_t* segment_ids,
    const uint8_t* accept_mask, uint32_t n_segments, uint8_t* prep_msgs_out, uint8_t* status_out,
    uint8_t* agg_shares_out, uint64_t* counts_out, int notify_fd, prio3_ticket** ticket_out);
int prio3_helper_aggregate_init_batch_ex_submit(
    prio3_engine* engine, struct janus_hpke_opener* opener,
    struct janus_hpke_opener* fallback_opener, uint64_t report_deadline, uint32_t n,
    const uint8_t task_id[32], int require_taskprov, const uint8_t* report_ids,
    const uint64_t* times, const uint8_t* public_shares, const uint8_t* enc, const uint8_t* ct,
    const uint32_t* ct_len, uint32_t ct_stride, const uint8_t* leader_prep_shares,
    const uint32_t* segment_ids, const uint8_t* accept_mask, uint32_t n_segments,
    uint8_t* prep_msgs_out, uint8_t* status_out, uint8_t* agg_shares_out, uint64_t* counts_out,
    int notify_fd, prio3_ticket** ticket_out);
int prio3_helper_aggregate_job_submit(prio3_engine* engine, const prio3_helper_job_in* job,
                                      const prio3_helper_job_out* out, int notify_fd,
                                      prio3_ticket** ticket_out);
/* *batch_out (nullable pointer) is filled by the wait */
int prio3_leader_prepare_init_batch_submit(prio3_engine* engine, uint32_t n, const uint8_t* nonces,
                                           const uint8_t* public_shares,
                                           const uint8_t* leader_input_shares,
                                           uint8_t* prep_shares_out, uint8_t* status_out,
                                           prio3_batch** batch_out, int notify_fd,
                                           prio3_ticket** ticket_out);
int prio3_leader_finish_job_submit(prio3_batch* batch, const prio3_leader_job_in* job,
                                   const prio3_leader_job_out* out, int notify_fd,
                                   prio3_ticket** ticket_out);
/* 1: the ticket's job is done (prio3_ticket_wait will not block), 0: pending.  Never blocks. */
int prio3_ticket_poll(const prio3_ticket* ticket);
/* Blocks until the job is done, writes its outputs, frees the ticket and returns what the blocking
 * call would have returned (PRIO3_EINVAL for a NULL ticket). */
int prio3_ticket_wait(prio3_ticket* ticket);

/* ---- Leader upload ---- */
/* The leader's upload handler for a batch of one task (VdafOps::handle_upload_generic,
 * aggregator/src/aggregator.rs:1522-1702; Janus batches the stored reports in ReportWriteBatcher):
 * from the uploaded `Report` bodies -- the rows prio3_client_prepare_reports_device writes,
 * reports[n][report_stride] with report_len[n] -- to the buffers the leader's prepare reads, with no
 * host parsing and no host cryptography.  Per report, the first failing check decides status[r]:
 *   1. the Report decodes (janus_dap_report_decode_*), else PRIO3_UPLOAD_MALFORMED (the handler's
 *      Error::MessageDecode, not a rejection);
 *   2. time > report_deadline (= now + tolerable clock skew, the caller's)   -> TooEarly (:1559)
 *   3. time > task_expiration (UINT64_MAX: none)                             -> TaskExpired (:1565)
 *   4. now > time + report_expiry_age (UINT64_MAX: none)                     -> Expired (:1572);
 *      a sum that overflows a u64 is PRIO3_UPLOAD_HOST (the reference's internal error)
 *   5. the public share's length is not prio3_sizes' public_share_len      -> DecodeFailure (:1588)
 *   6. the leader ciphertext's config ID is neither opener's  -> OutdatedHpkeConfig (:1626); the
 *      leader config IDs are written out so that the host can name the ID
 *   7. HPKE open over InputShareAad { task_id, metadata, public share } (built on the device) with
 *      the opener of that config ID; when both have it, the task's first and the global one only
 *      for a report whose open failed (:1637-1644)                         -> DecryptFailure
 *      (also: an `enc` that is not the KEM's Nenc bytes, a payload below 16 bytes)
 *   8. PlaintextInputShare::get_decoded and the Prio3 leader share (:1661-1686): the u16-prefixed
 *      extension list { u16 type, u16-prefixed data } is well formed (the codec's ExtensionType
 *      knows Tbd = 0 and Taskprov = 0xFF00; duplicates and the like are not the handler's), the
 *      u32-prefixed payload ends the plaintext, has leader_input_share_len bytes, and every field
 *      element of the measurement and proofs shares is canonical (LE Field128; Field64 for
 *      PRIO3_SUMVEC_F64_MP)                                                 -> DecodeFailure
 *   then PRIO3_UPLOAD_HOST when the extension bytes do not fit ext_stride: the host handles that
 *   report itself.
 * The codes are Janus's ReportRejectionReason in the order of aggregator/error.rs:220-228, from 1;
 * IntervalCollected is never produced here (that check stays in the writer's transaction).
 * Both openers (janus_hpke.h; either may be NULL, not both) are created with the info
 * "dap-09 input share" || 0x01 || 0x02 and are bound to the engine's GPU.
 * Outputs: report_ids[n][16], times[n], public_shares[n][public_share_len] (NULL when that is 0),
 * leader_input_shares[n][leader_input_share_len] -- what prio3_leader_prepare_init_batch /
 * prio3_device_leader_prepare_init read; extensions[n][ext_stride] with ext_len[n] (the encoded
 * list body, as LeaderStoredReport keeps it); the helper's ciphertext as the rows
 * janus_dap_agg_init_req_encode_* reads (helper_config_ids[n], helper_enc[n][helper_enc_len],
 * helper_ct[n][helper_ct_stride], helper_ct_len[n]; janus_dap.h); leader_config_ids[n]; status[n].
 * Every row of a report with a non-zero status is zero (its leader config ID excepted, unless the
 * Report is malformed), and a failed open leaves no plaintext behind, in scratch either.
 * PRIO3_EINVAL: both openers NULL, an opener on another GPU than the engine, report_stride or
 * ext_stride not a multiple of 4 (d_reports 4-byte aligned), a missing buffer.
 * PRIO3_FPVEC_BOUNDED_L2 returns PRIO3_EUNSUPPORTED.  Engine option upload_aead: 0 chooses the AEAD
 * kernel by the instance's payload length, 1 forces the one-lane body of the helper's open, 2 the
 * 16-lanes-per-report AES-GCM kernel; ChaCha20Poly1305 always takes the one-lane body.
 * Device form: stream-ordered, no host synchronisation, scratch from the GPU's pool (batches above
 * 65536 reports run in sub-batches on the stream); the calling thread's device is left as it was.
 * Host form: a plain blocking call. */
enum {
  PRIO3_UPLOAD_OK = 0,
  PRIO3_UPLOAD_INTERVAL_COLLECTED = 1,
  PRIO3_UPLOAD_DECRYPT_FAILURE = 2,
  PRIO3_UPLOAD_DECODE_FAILURE = 3,
  PRIO3_UPLOAD_TASK_EXPIRED = 4,
  PRIO3_UPLOAD_EXPIRED = 5,
  PRIO3_UPLOAD_TOO_EARLY = 6,
  PRIO3_UPLOAD_OUTDATED_HPKE_CONFIG = 7,
  PRIO3_UPLOAD_MALFORMED = 0x40,
  PRIO3_UPLOAD_HOST = 0x41,
};
int prio3_device_leader_upload(
    prio3_engine* engine, struct janus_hpke_opener* task_opener, uint8_t task_config_id,
    struct janus_hpke_opener* global_opener, uint8_t global_config_id, uint32_t n,
    const uint8_t task_id[32], uint64_t now, uint64_t report_deadline, uint64_t task_expiration,
    uint64_t report_expiry_age, const uint8_t* d_reports, uint32_t report_stride,
    const uint32_t* d_report_len, uint8_t* d_report_ids, uint64_t* d_times,
    uint8_t* d_public_shares, uint8_t* d_leader_input_shares, uint8_t* d_extensions,
    uint32_t* d_ext_len, uint32_t ext_stride, uint8_t* d_helper_config_ids, uint8_t* d_helper_enc,
    uint32_t helper_enc_len, uint8_t* d_helper_ct, uint32_t* d_helper_ct_len,
    uint32_t helper_ct_stride, uint8_t* d_leader_config_ids, uint8_t* d_status, void* stream);
int prio3_leader_upload_batch(
    prio3_engine* engine, struct janus_hpke_opener* task_opener, uint8_t task_config_id,
    struct janus_hpke_opener* global_opener, uint8_t global_config_id, uint32_t n,
    const uint8_t task_id[32], uint64_t now, uint64_t report_deadline, uint64_t task_expiration,
    uint64_t report_expiry_age, const uint8_t* reports, uint32_t report_stride,
    const uint32_t* report_len, uint8_t* report_ids, uint64_t* times, uint8_t* public_shares,
    uint8_t* leader_input_shares, uint8_t* extensions, uint32_t* ext_len, uint32_t ext_stride,
    uint8_t* helper_config_ids, uint8_t* helper_enc, uint32_t helper_enc_len, uint8_t* helper_ct,
    uint32_t* helper_ct_len, uint32_t helper_ct_stride, uint8_t* leader_config_ids,
    uint8_t* status);
/* The job form: prio3_leader_upload_batch through the upload executor (kind 5 of
 * prio3_executor_stats_get / prio3_executor_control).  Concurrent jobs -- of any task, each with its
 * own task ID, now, report_deadline, task_expiration and report_expiry_age -- share one launch chain
 * when they name the same two openers and config IDs, the same report_stride, ext_stride,
 * helper_enc_len and helper_ct_stride, and engines of one VDAF instance with the same upload_aead
 * choice.  Each job copies its rows once, into its group's pinned staging, on the calling thread.
 * The fields of prio3_upload_job_in are the inputs of prio3_leader_upload_batch under the same names
 * (task_id: the 32 bytes themselves), those of prio3_upload_job_out its twelve host output pointers,
 * with the same nullability rules (public_shares, extensions, helper_enc, helper_ct: NULL when their
 * row length is 0).  Every output is byte for byte what prio3_leader_upload_batch writes for the
 * same arguments, and so are the return codes: PRIO3_EINVAL for a NULL engine, job or out, both
 * openers NULL, an opener on another GPU than the engine, report_stride or ext_stride not a multiple
 * of 4, report_stride >= 2^31, helper_enc_len > 0xFFFF, a missing buffer (n > 0);
 * PRIO3_EUNSUPPORTED for PRIO3_FPVEC_BOUNDED_L2; n == 0 is PRIO3_OK.
 * prio3_leader_upload_job_submit is its ticketed twin and obeys the rules of "Ticketed job
 * submission" above word for word: the inputs -- the rows, the lengths and both structs -- are read
 * only inside the submit call, the outputs are written only inside prio3_ticket_wait on the waiting
 * thread, notify_fd is written exactly once per ticket, prio3_ticket_poll never blocks, and the
 * calling thread's HIP device is left as it was.  The helper's ciphertext rows are cut out of the
 * job's staged Report rows inside the wait: they cross the link once, inside the Report.
 * Synchronous paths (prio3_leader_upload_batch runs inside the call, or inside submit with a done
 * ticket and notify_fd written there): an empty job; a job of more than
 * PRIO3_UPLOAD_JOB_MAX_REPORTS reports; rows that do not fit one group's staging; an engine with
 * option coalesce = 0.  No size or instance is refused that the batch form accepts.  A multi-GPU
 * engine places the job on its least-loaded member on the openers' GPU.
 * PRIO3_UPLOAD_JOB_MAX_REPORTS: a group's pinned staging is 96 MB and holds, per report, the Report
 * row and every output row but the helper's (report_stride + public_share_len +
 * leader_input_share_len + ext_stride + 83 bytes); the limit is 96 MB over the largest such
 * footprint a job may have and still coalesce whatever its size, 24 KB -- about twice that of a
 * Histogram(256,16) report (a 5.7 KB row and a 5.6 KB leader share).  A job with a larger footprint
 * coalesces while n times the footprint is within the staging. */
enum { PRIO3_UPLOAD_JOB_MAX_REPORTS = 4096 };
typedef struct {
  struct janus_hpke_opener* task_opener;   /* nullable (not both) */
  struct janus_hpke_opener* global_opener; /* nullable (not both) */
  uint8_t task_config_id;
  uint8_t global_config_id;
  uint8_t reserved[2];                     /* 0 */
  uint32_t n;
  uint8_t task_id[32];
  uint64_t now;
  uint64_t report_deadline;
  uint64_t task_expiration;                /* UINT64_MAX: none */
  uint64_t report_expiry_age;              /* UINT64_MAX: none */
  const uint8_t* reports;                  /* host [n][report_stride] */
  const uint32_t* report_len;              /* host [n] */
  uint32_t report_stride;
  uint32_t ext_stride;
  uint32_t helper_enc_len;
  uint32_t helper_ct_stride;
} prio3_upload_job_in;
typedef struct {
  uint8_t* report_ids;                     /* [n][16] */
  uint64_t* times;                         /* [n] */
  uint8_t* public_shares;                  /* [n][public_share_len] */
  uint8_t* leader_input_shares;            /* [n][leader_input_share_len] */
  uint8_t* extensions;                     /* [n][ext_stride] */
  uint32_t* ext_len;                       /* [n] */
  uint8_t* helper_config_ids;              /* [n] */
  uint8_t* helper_enc;                     /* [n][helper_enc_len] */
  uint8_t* helper_ct;                      /* [n][helper_ct_stride] */
  uint32_t* helper_ct_len;                 /* [n] */
  uint8_t* leader_config_ids;              /* [n] */
  uint8_t* status;                         /* [n] */
} prio3_upload_job_out;
int prio3_leader_upload_job(prio3_engine* engine, const prio3_upload_job_in* job,
                            const prio3_upload_job_out* out);
int prio3_leader_upload_job_submit(prio3_engine* engine, const prio3_upload_job_in* job,
                                   const prio3_upload_job_out* out, int notify_fd,
                                   prio3_ticket** ticket_out);

/* ---- Client ---- */
/* The client role of prio::vdaf: Prio3::shard on the caller's measurements (client/src/lib.rs:
 * 339-341), for Count, Sum, SumVec, Histogram and SumVecField64MultiproofHmacSha256Aes128
 * (PRIO3_SUMVEC_F64_MP).  Per report r: d_measurements[r][SumVec and the multiproof SumVec:
 * length, else 1] (u64), d_nonces[r][16] (the report ID) and d_rand[r][prio3_client_rand_len] from
 * the caller's CSPRNG (the library draws no randomness, and a row must never be reused).
 * Randomness layout, prio's order, seeds of the instance's XOF seed size -- 16 bytes
 * (XofTurboShake128), 32 bytes for PRIO3_SUMVEC_F64_MP (XofHmacSha256Aes128: 160 bytes per report):
 *   helper measurement share seed | helper proofs share seed |
 *   [ helper blind | leader blind | ]  prove randomness seed
 * -- the two blinds only for instances with joint randomness (Sum, SumVec, the multiproof SumVec,
 * Histogram: joint_rand_len of prio3_sizes non-zero); without them (Count) the prove seed follows
 * the two helper seeds.
 * Outputs per report: d_public_shares[r][public_share_len] (may be NULL when that is 0),
 * d_leader_input_shares[r][leader_input_share_len], d_helper_shares[r][helper_share_len] and
 * d_status[r]: PRIO3_CLIENT_OK, or PRIO3_CLIENT_INVALID_MEASUREMENT for a measurement prio's
 * encode_measurement rejects (Count: not 0 / 1; Sum, SumVec, the multiproof SumVec: an entry
 * >= 2^bits; Histogram: an index >= length) -- its three rows are all zero and the other reports
 * are not affected.  The multiproof instance's leader input share holds the measurement share, then
 * all num_proofs proof shares (little-endian Field64), then the 32-byte leader blind; its public
 * share is the two 32-byte joint-rand parts, the leader's first.
 * Every XOF expansion is sampled exactly (rejection sampling as prio does; there is no "unusable"
 * flag as in the synthetic generator below), the engine's verify key is not read, and nothing of
 * the leader's prepare_init is computed.  Device pointers are 16-byte aligned.  Stream-ordered;
 * the call does not wait for the device.
 * PRIO3_FPVEC_BOUNDED_L2 returns PRIO3_EUNSUPPORTED from every entry point of this section (its
 * circuit is a reconstruction and its fixed-point encoding needs a contract of its own); its
 * seeded generator below stays. */
enum { PRIO3_CLIENT_OK = 0, PRIO3_CLIENT_INVALID_MEASUREMENT = 1 };
/* seed_size * (5 with joint randomness, else 3); 0 for parameters prio3_sizes rejects */
int prio3_client_rand_len(const prio3_params* params);
int prio3_client_shard_device(prio3_engine* engine, uint32_t n, const uint64_t* d_measurements,
                              const uint8_t* d_nonces, const uint8_t* d_rand,
                              uint8_t* d_public_shares, uint8_t* d_leader_input_shares,
                              uint8_t* d_helper_shares, uint8_t* d_status, void* stream);
/* The same with host buffers (blocking). */
int prio3_client_shard_batch(prio3_engine* engine, uint32_t n, const uint64_t* measurements,
                             const uint8_t* nonces, const uint8_t* rand, uint8_t* public_shares,
                             uint8_t* leader_input_shares, uint8_t* helper_shares,
                             uint8_t* status);

/* Client::prepare_report (client/src/lib.rs:339-383) for a batch of one task, on one stream with
 * no host round trip: each time rounded down to the task's time precision (t - t % precision,
 * to_batch_interval_start), the shard above, one input share sealed to each aggregator -- the
 * leader's with leader_sealer (info "dap-09 input share" || 0x01 || 0x02), the helper's with
 * helper_sealer (... || 0x01 || 0x03), both over the same InputShareAad { task_id, metadata,
 * public share } with the rounded time, each with its own caller-supplied ephemeral keys
 * d_sk_e_leader / d_sk_e_helper [n][32] (janus_hpke.h, Seal) -- and the Report encode of
 * janus_dap.h.  The client sends no extension (lib.rs:361); with_taskprov_extension adds the one
 * empty taskprov extension to both plaintexts, as janus_hpke_seal_input_shares_device does.
 * Outputs: d_reports[n][report_stride] with d_report_len[n] (u32), and d_status[n]: 0,
 * PRIO3_CLIENT_INVALID_MEASUREMENT, or the sealer's JANUS_HPKE_SEAL_KEY_ERROR (0x40) /
 * _LENGTH_ERROR (0x41), the shard's first, then the leader seal's; a report with a non-zero status
 * has length 0 and a zero row.  report_stride >= prio3_client_report_stride(...), else
 * PRIO3_EINVAL; also PRIO3_EINVAL: time_precision 0, a NULL sealer, a sealer bound to another GPU
 * than the engine.  (A sealer exists only for the KEMs the seal supports: X25519 and P-256.)
 * The intermediate shares and ciphertexts live in pooled device scratch; batches whose scratch
 * does not fit in free memory run in sub-batches on the same stream. */
struct janus_hpke_sealer;
/* the row length that holds any Report of the instance and the two sealers' KEMs (0: invalid
 * parameters or a NULL sealer) */
int prio3_client_report_stride(const prio3_params* params,
                               const struct janus_hpke_sealer* leader_sealer,
                               const struct janus_hpke_sealer* helper_sealer,
                               int with_taskprov_extension);
int prio3_client_prepare_reports_device(
    prio3_engine* engine, struct janus_hpke_sealer* leader_sealer,
    struct janus_hpke_sealer* helper_sealer, uint32_t n, const uint8_t task_id[32],
    uint64_t time_precision, const uint64_t* d_measurements, const uint8_t* d_report_ids,
    const uint64_t* d_times, const uint8_t* d_rand, const uint8_t* d_sk_e_leader,
    const uint8_t* d_sk_e_helper, uint8_t leader_config_id, uint8_t helper_config_id,
    int with_taskprov_extension, uint8_t* d_reports, uint32_t report_stride,
    uint32_t* d_report_len, uint8_t* d_status, void* stream);

/* ---- Synthetic client (benchmarks and tests) ---- */
/* Generates n honest reports on the device: the client's shard (prio Prio3::shard,
 * client/src/lib.rs:339-341) and the leader's prepare_init (agg_id 0,
 * aggregation_job_driver.rs:397-415), for the engine's instance and verify key.  Report i is
 * derived from (seed, first_index + i) exactly like the oracle's generator.
 * d_measurements: n x (SumVec: length, else 1) u64 (nullable); d_leader_out_shares:
 * n x agg_share_len (nullable); d_flags: n bytes, non-zero if a rejection-sampling event made
 * the report unusable (nullable); d_leader_input_shares: n x leader_input_share_len, the
 * leader's input shares for the leader-side entry points (nullable). */
int prio3_client_generate_device(prio3_engine* engine, uint32_t n, uint64_t seed,
                                 uint64_t first_index, uint8_t* d_nonces,
                                 uint8_t* d_public_shares, uint8_t* d_helper_shares,
                                 uint8_t* d_leader_prep_shares, uint64_t* d_measurements,
                                 uint8_t* d_leader_out_shares, uint8_t* d_flags,
                                 uint8_t* d_leader_input_shares, void* stream);

/* Frees the idle scratch slabs the device's pool keeps for later calls (up to 1/8 of HBM, shared
 * by every engine on the GPU; a run an engine or a batch handle still references stays).  For a
 * process that hands the GPU's memory to something else between batches. */
int prio3_device_trim(int device);

/* ---- Test / measurement knobs ---- */
/* force_slow_path=1 routes every report through the general rejection-sampling kernel;
 * leader_fuse_acc=0 turns off the fused device-leader accumulate (A/B); pair_max=N runs
 * Histogram(P = 32) prepares of at most N reports on lane pairs (0: never); the other keys are
 * the launch variants prio3_engine_set_option (prio3_engine.hip) lists.  test_reject_bits=N
 * (0..24) exists only in the test-rejection build (libjanus_prio3_rej.so); elsewhere it fails. */
int prio3_engine_set_option(prio3_engine* engine, const char* key, int64_t value);
/* Per-kernel device time (ms) accumulated since the last reset, measured with HIP events
 * on the launch stream when option "timing" is 1 (2: launches counted, no events or times).
 * names: comma-separated kernel names. */
int prio3_engine_timing(prio3_engine* engine, char* names, size_t names_cap, double* ms,
                        uint64_t* launches, int cap);
void prio3_engine_timing_reset(prio3_engine* engine);
/* 1 if the entry points emit roctx ranges (environment JANUS_ROCTX=1 when the library was first
 * used and a roctx library loadable): "handle_aggregate_init_generic threadpool task" around
 * prio3_helper_prepare_batch, "VDAF preparation" around the device prepares, "batch aggregation"
 * around the accumulates -- the spans of aggregator.rs:1786-1790, 2021. */
int prio3_trace_enabled(void);

/* Test-only: runs one Field128 primitive of the device library over n host-supplied operand
 * pairs (16-byte LE elements) -- op 0/1: a*b (compiler / hand-scheduled), 2: a+b, 3: a-b,
 * 4/5: sum of 16 products per output through the lazily reduced MAC (a, b hold 16 n elements).
 * Lets tests pin the hand-written asm arithmetic against Python integers directly. */
int prio3_selftest_field(int op, uint32_t n, const uint8_t* a, const uint8_t* b, uint8_t* out);

/* Test-only: Field64 primitives and the limit-operand pieces of Field128, one result per i < n.
 * op 0/1/2: a*b, a+b, a-b in Field64 (8-byte LE a, b, out);  3: the reduction of the raw 128-bit
 * value lo = a[i], hi = b[i];  4: sum of k products per output through the lazily reduced Field64
 * MAC (a, b hold k n elements);  5: 1 if the raw a[i] < p64, else 0;  6: the same for a raw
 * 16-byte a[i] and p128 (8-byte out);  7: a[i] added k times through the lazy Field128 sum, then
 * reduced (16-byte a, out; b unused from op 5 on);  8: the measurement-share truncation with
 * nb = k <= 32 over two entries: a holds 2 k n 16-byte elements (lane i's at 2 k i), out the
 * entries as [2][n] 16-byte elements. */
int prio3_selftest_field64(int op, uint32_t n, uint32_t k, const uint8_t* a, const uint8_t* b,
                           uint8_t* out);

/* Test-only: runs the fused accumulate's tile reduction on one wave's host-supplied values.
 * values: [8][64][16 B], slot-major (slot s of lane l at (s * 64 + l) * 16, LE Field128 words);
 * all 8 slots are staged, the first n_elems (1..8) are reduced.  out: [n_elems][8] uint32, the 8
 * addends of each slot's sum over the 64 lanes, addend h at weight 2^(16 h), each < 2^22. */
int prio3_selftest_tile(uint32_t n_elems, const uint8_t* values, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif
