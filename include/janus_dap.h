/*
 * janus_dap.h -- C ABI of the DAP wire-format <-> SoA marshaling around the device calls
 * (SURVEY.md 8(f) row 3), MI355X (gfx950).
 *
 * Helper side of an aggregation job, DAP-09 encodings of /root/reference/messages/src/lib.rs:
 *   AggregationJobInitializeReq (lib.rs:2362-2400) = u32-prefixed aggregation parameter,
 *     PartialBatchSelector (query type byte, + 32-byte BatchId for FixedSize),
 *     u32-prefixed list of PrepareInit (lib.rs:2021-2070):
 *       ReportShare { ReportMetadata { report_id[16], time u64 }, u32-prefixed public share,
 *                     HpkeCiphertext { config_id u8, u16-prefixed enc, u32-prefixed payload } }
 *       u32-prefixed PingPongMessage (type u8, u32-prefixed prep_share for Initialize)
 *   AggregationJobResp (lib.rs:2535-2550) = u32-prefixed list of PrepareResp { report_id,
 *     PrepareStepResult: 0 Continue { u32-prefixed PingPongMessage } | 1 Finished |
 *     2 Reject(PrepareError u8) }  (lib.rs:2130-2190)
 *
 * These replace Janus's per-report decode (`AggregationJobInitializeReq::get_decoded`,
 * aggregator.rs:1720-1790) and the response assembly (aggregator.rs:2044-2096, 2140-2170):
 * the request body is unpacked on the device straight into the SoA buffers
 * janus_hpke_open_input_shares_device and prio3_device_prepare_aggregate read, and the response
 * body is encoded on the device from their outputs.
 *
 * Unpack is speculative: when every PrepareInit of the body has the byte length of the first
 * one (one VDAF, one HPKE suite, same extensions -- the normal case) the device parses all of
 * them in parallel and validates each; any record that does not fit is reported and the caller
 * uses the host parser (janus_dap_agg_init_unpack_host) for the body.
 */
#ifndef JANUS_DAP_H
#define JANUS_DAP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { JANUS_DAP_QUERY_TIME_INTERVAL = 1, JANUS_DAP_QUERY_FIXED_SIZE = 2 };

/* Per-report message status written by unpack (prio3 status codes, janus_prio3.h): 0 = the
 * message is PingPongMessage::Initialize with a prep_share of the expected length;
 * 2 = CodecPrepShare (wrong prep_share length); 5 = PeerMessageMismatch (Continue / Finish);
 * 6 = the public share has another length than layout->public_share_len -- it does not decode:
 * PrepareError::InvalidMessage (aggregator.rs:1985-1999), after any HPKE error of the report.
 * A PingPongMessage that does not decode (unknown type, bad framing) rejects the whole request,
 * as Janus's request decode does.  janus_dap_agg_init_scan_ex takes the lengths the task
 * expects (VDAF public share, KEM Nenc, VDAF prep share), so a malformed first record fails
 * alone; janus_dap_agg_init_scan takes them from the first record. */

typedef struct {
  /* filled by janus_dap_agg_init_scan */
  uint32_t n;                   /* number of PrepareInits (valid after unpack_host; for the
                                   device path n = list bytes / record_len) */
  uint8_t query_type;           /* JANUS_DAP_QUERY_* */
  uint8_t batch_id[32];         /* FixedSize only */
  uint64_t agg_param_off, agg_param_len;
  uint64_t list_off, list_len;  /* byte range of the PrepareInit list */
  uint32_t record_len;          /* byte length of the first PrepareInit */
  uint32_t public_share_len;    /* expected (scan_ex) or of the first record */
  uint32_t enc_len, payload_len, message_len, prep_share_len;  /* enc / prep share: as
                                   public_share_len; payload, message: of the first record */
  int uniform;                  /* list_len is a multiple of record_len */
} janus_dap_agg_init_layout;

/* Parses the header and the first PrepareInit of an AggregationJobInitializeReq body (host
 * memory; O(1)).  Returns 0, or -1 if the header does not decode. */
int janus_dap_agg_init_scan(const uint8_t* body, size_t len, janus_dap_agg_init_layout* out);

/* As janus_dap_agg_init_scan, with the lengths every record must have: the VDAF's public share
 * length, the HPKE KEM's Nenc and the VDAF's leader prep share length (JANUS_DAP_LEN_ANY: the
 * first record's).  The layout carries the expected lengths; if the first record differs from
 * them, layout->uniform is 0 and the caller unpacks on the host, where each record with another
 * public share / prep share length gets msg_status 6 / 2 and another enc length ct_len 0 (HPKE
 * decrypt error) -- the reference fails only that report (aggregator.rs:1967-1999). */
#define JANUS_DAP_LEN_ANY 0xFFFFFFFFu
int janus_dap_agg_init_scan_ex(const uint8_t* body, size_t len, uint32_t public_share_len,
                               uint32_t enc_len, uint32_t prep_share_len,
                               janus_dap_agg_init_layout* out);

/* Device unpack of a body whose records all have layout->record_len bytes (layout->uniform).
 * d_body is the request body in device memory.  Outputs (device, n = list_len / record_len):
 *   d_report_ids[n][16], d_times[n] (seconds), d_public_shares[n][public_share_len],
 *   d_config_ids[n], d_enc[n][enc_len], d_ct[n][ct_stride] + d_ct_len[n] (the HPKE payload),
 *   d_prep_shares[n][prep_share_len] (leader prep share), d_msg_status[n].
 * ct_stride must be >= payload_len and a multiple of 16.  *d_mismatch (device u32, zeroed here)
 * counts the records that do not have the first record's shape; when it is non-zero the outputs
 * are incomplete and the caller must use janus_dap_agg_init_unpack_host. */
int janus_dap_agg_init_unpack_device(const janus_dap_agg_init_layout* layout, const uint8_t* d_body,
                                     uint8_t* d_report_ids, uint64_t* d_times,
                                     uint8_t* d_public_shares, uint8_t* d_config_ids,
                                     uint8_t* d_enc, uint8_t* d_ct, uint32_t* d_ct_len,
                                     uint32_t ct_stride, uint8_t* d_prep_shares,
                                     uint8_t* d_msg_status, uint32_t* d_mismatch, void* stream);

/* Host (sequential) unpack of any well-formed body into host SoA buffers sized for `cap`
 * records: prep shares / public shares of another length than the first record's get
 * msg_status 2 / 6 (the public share row is zero-filled);
 * payloads longer than ct_stride give ct_len 0 (HPKE decrypt error).  Returns the number of
 * records, or -1 if the body does not decode (the whole request is rejected, as Janus does). */
int64_t janus_dap_agg_init_unpack_host(const uint8_t* body, size_t len,
                                       const janus_dap_agg_init_layout* layout, uint32_t cap,
                                       uint8_t* report_ids, uint64_t* times,
                                       uint8_t* public_shares, uint8_t* config_ids, uint8_t* enc,
                                       uint8_t* ct, uint32_t* ct_len, uint32_t ct_stride,
                                       uint8_t* prep_shares, uint8_t* msg_status);

/* AggregationJobResp for the helper's init step.  Per report the PrepareStepResult is
 *   prepare_error[r] != 0xFF  -> Reject(prepare_error[r])       (HPKE / decode / host checks)
 *   else prio3_status[r] == 0 -> Continue { PingPongMessage::Finish { prep_msg[r] } }
 *   else                      -> Reject(VdafPrepError = 5)        (handle_ping_pong_error)
 * Device form: d_out must hold janus_dap_agg_job_resp_max_len(n, prep_msg_len) bytes;
 * *d_out_len (device u64) receives the encoded length.  d_scratch: 4 * (n / 256 + 2) bytes. */
size_t janus_dap_agg_job_resp_max_len(uint32_t n, uint32_t prep_msg_len);
int janus_dap_agg_job_resp_encode_device(uint32_t n, const uint8_t* d_report_ids,
                                         const uint8_t* d_prepare_error,
                                         const uint8_t* d_prio3_status, const uint8_t* d_prep_msgs,
                                         uint32_t prep_msg_len, uint8_t* d_out,
                                         uint64_t* d_out_len, uint32_t* d_scratch, void* stream);
int64_t janus_dap_agg_job_resp_encode_host(uint32_t n, const uint8_t* report_ids,
                                           const uint8_t* prepare_error,
                                           const uint8_t* prio3_status, const uint8_t* prep_msgs,
                                           uint32_t prep_msg_len, uint8_t* out);

/* ---- Leader side: the two opposite directions --------------------------------------------
 * The leader encodes the AggregationJobInitializeReq from the SoA buffers its device calls hold
 * (report metadata, public shares, the HPKE ciphertexts of the helper input shares as
 * janus_hpke_seal_input_shares_device writes them, and the prepare shares of
 * prio3_device_leader_prepare_init) and decodes the helper's AggregationJobResp into the prepare
 * messages prio3_device_leader_prepare_next reads -- Janus's loops at
 * aggregation_job_driver.rs:417-437 and :657-752.
 *
 * Request encode.  A report with leader_status[r] != 0 is left out (the driver `continue`s past
 * a report whose leader_initialized failed, :430-437).  index[r] receives the report's position
 * in the request or JANUS_DAP_INDEX_NONE (the driver's stepped_aggregations); the response decode
 * reads it.  Every PingPongMessage is Initialize { prep_shares[r] }.  enc_len must fit a u16.
 *
 * Host form: returns the body's length, or JANUS_DAP_EARG (a null pointer, an unknown query type,
 * a ct_len above ct_stride) or JANUS_DAP_ETOOLONG (the PrepareInit list does not fit its u32
 * length prefix; nothing usable is written).  out must hold
 * janus_dap_agg_init_req_max_len(...) bytes.
 *
 * Device form: agg_param and batch_id are host memory (agg_param_len <= JANUS_DAP_AGG_PARAM_MAX;
 * Prio3's is empty), every d_ pointer is device memory.  d_ct / d_ct_len are the rows the
 * device sealer writes; a report whose ct_len is above ct_stride is left out like a failed one
 * and counted in d_err[0], and no byte past a row is read.  d_err[1] is 1 when the list does not
 * fit a u32: *d_out_len and *d_n_included are then 0 and the body is not written.  d_scratch:
 * 4 * n + 16 * (n / 256 + 2) bytes, 8-byte aligned.  Runs on `stream` of the GPU that owns d_out, without
 * host synchronisation; the calling thread's current device is left as it was. */
#define JANUS_DAP_INDEX_NONE 0xFFFFFFFFu
#define JANUS_DAP_AGG_PARAM_MAX 256
enum { JANUS_DAP_EARG = -1, JANUS_DAP_EDEVICE = -2, JANUS_DAP_ETOOLONG = -3 };

size_t janus_dap_agg_init_req_max_len(uint32_t n, uint32_t agg_param_len, uint8_t query_type,
                                      uint32_t public_share_len, uint32_t enc_len,
                                      uint32_t ct_stride, uint32_t prep_share_len);
int64_t janus_dap_agg_init_req_encode_host(uint32_t n, const uint8_t* agg_param,
                                           uint32_t agg_param_len, uint8_t query_type,
                                           const uint8_t* batch_id, const uint8_t* report_ids,
                                           const uint64_t* times, const uint8_t* public_shares,
                                           uint32_t public_share_len, const uint8_t* config_ids,
                                           const uint8_t* enc, uint32_t enc_len, const uint8_t* ct,
                                           const uint32_t* ct_len, uint32_t ct_stride,
                                           const uint8_t* prep_shares, uint32_t prep_share_len,
                                           const uint8_t* leader_status, uint8_t* out,
                                           uint32_t* index, uint32_t* n_included);
int janus_dap_agg_init_req_encode_device(uint32_t n, const uint8_t* agg_param,
                                         uint32_t agg_param_len, uint8_t query_type,
                                         const uint8_t* batch_id, const uint8_t* d_report_ids,
                                         const uint64_t* d_times, const uint8_t* d_public_shares,
                                         uint32_t public_share_len, const uint8_t* d_config_ids,
                                         const uint8_t* d_enc, uint32_t enc_len,
                                         const uint8_t* d_ct, const uint32_t* d_ct_len,
                                         uint32_t ct_stride, const uint8_t* d_prep_shares,
                                         uint32_t prep_share_len, const uint8_t* d_leader_status,
                                         uint8_t* d_out, uint64_t* d_out_len, uint32_t* d_index,
                                         uint32_t* d_n_included, uint32_t* d_err, void* d_scratch,
                                         void* stream);

/* Response decode, in the engine's row order through index[] (n rows, n_included of them in the
 * request).  prep_msgs[n][prep_msg_len]: a row is all zero unless its report continued.
 * prepare_error[n]: 0xFF = the helper continued and the row holds its prepare message; any other
 * value is the DAP PrepareError the report fails with.  A row with index[r] ==
 * JANUS_DAP_INDEX_NONE keeps 0xFF and a zero row (its failure is in the caller's leader status).
 * Per PrepareResp (aggregation_job_driver.rs:673-752):
 *   Continue { Finish { prep_msg } } of prep_msg_len bytes -> 0xFF and the row
 *   Reject(e), e <= 9                                       -> e
 *   Finished                                                -> 5 (VdafPrepError, :714-732)
 *   Continue with Initialize / Continue, or a Finish of another length -> 5 (:677-710)
 * The whole response is rejected when it does not decode (a Reject code above 9, lib.rs:2185-2196,
 * included), when its record count is not n_included or when a record's report ID is not the
 * expected one at that position (:657-671).
 *
 * Host form: returns 0 or one of the JANUS_DAP_RESP_E* codes.  It decodes the whole body first
 * (ELISTLEN, ETRAILING, EMALFORMED, EREJECT_CODE), then compares the count (ECOUNT) and the IDs
 * (EID).
 *
 * Device form: speculative, like the request unpack.  It decodes any mix of the three regular
 * shapes (Continue-Finish of prep_msg_len bytes, Finished, Reject) with no host help; any other
 * record stops it with JANUS_DAP_RESP_IRREGULAR in *d_flags (and JANUS_DAP_RESP_MALFORMED when
 * the record cannot decode) and the caller uses the host form.  *d_flags (device u32, zeroed
 * here) is the OR of the JANUS_DAP_RESP_* bits; when it is non-zero the outputs are incomplete.
 * d_body must be readable up to a dword past body_len.  d_scratch: 8 * (n_included + 2) bytes,
 * 4-byte aligned.  Stream and device as for the request encode (the GPU that owns d_flags). */
enum {
  JANUS_DAP_RESP_IRREGULAR = 1,   /* a record of another shape: use the host form */
  JANUS_DAP_RESP_LISTLEN = 2,     /* the list length runs past the body */
  JANUS_DAP_RESP_TRAILING = 4,    /* bytes after the list */
  JANUS_DAP_RESP_MALFORMED = 8,   /* a record or its PingPongMessage does not decode */
  JANUS_DAP_RESP_REJECT_CODE = 16, /* Reject with a code above 9 */
  JANUS_DAP_RESP_COUNT = 32,      /* the record count is not n_included */
  JANUS_DAP_RESP_ID = 64          /* a record's report ID is not the expected one */
};
enum {
  JANUS_DAP_RESP_ELISTLEN = -3,
  JANUS_DAP_RESP_ETRAILING = -4,
  JANUS_DAP_RESP_EMALFORMED = -5,
  JANUS_DAP_RESP_EREJECT_CODE = -6,
  JANUS_DAP_RESP_ECOUNT = -7,
  JANUS_DAP_RESP_EID = -8
};
int janus_dap_agg_job_resp_unpack_host(uint32_t n, const uint32_t* index,
                                       const uint8_t* report_ids, uint32_t n_included,
                                       const uint8_t* body, size_t body_len, uint32_t prep_msg_len,
                                       uint8_t* prep_msgs, uint8_t* prepare_error);
int janus_dap_agg_job_resp_unpack_device(uint32_t n, const uint32_t* d_index,
                                         const uint8_t* d_report_ids, uint32_t n_included,
                                         const uint8_t* d_body, size_t body_len,
                                         uint32_t prep_msg_len, uint8_t* d_prep_msgs,
                                         uint8_t* d_prepare_error, uint32_t* d_flags,
                                         void* d_scratch, void* stream);

/* ---- Client side: the upload body -----------------------------------------------------------
 * Report (lib.rs, struct Report) = ReportMetadata { report_id[16], time u64 }, u32-prefixed
 * public share, HpkeCiphertext to the leader, HpkeCiphertext to the helper -- what
 * Client::prepare_report returns (client/src/lib.rs:339-383) and the client PUTs to the leader.
 * Every report is its own HTTP body, so the output is one row per report: out[n][out_stride] and
 * out_len[n] (u32).  The ciphertext rows are those the sealer writes (enc[n][enc_len],
 * ct[n][ct_stride] with ct_len[n]); no byte past a row's ct_len is read.  A report whose skip byte
 * is non-zero (skip may be NULL), or one of whose ct_len is 0 or above its stride, is left out:
 * out_len 0 and an all-zero row.  The bytes of a row past its report are zero.  out_stride below
 * janus_dap_report_max_len(...) or an enc_len above 0xFFFF is JANUS_DAP_EARG.
 * Device form: runs on `stream` of the GPU that owns d_out without host synchronisation; the
 * calling thread's current device is left as it was.  Host form: returns the number of reports
 * written (rows with out_len != 0) or JANUS_DAP_EARG.  The decoding direction (the leader's upload
 * handler) is janus_dap_report_decode_* below. */
size_t janus_dap_report_max_len(uint32_t public_share_len, uint32_t leader_enc_len,
                                uint32_t leader_ct_stride, uint32_t helper_enc_len,
                                uint32_t helper_ct_stride);
int janus_dap_report_encode_device(uint32_t n, const uint8_t* d_report_ids, const uint64_t* d_times,
                                   const uint8_t* d_public_shares, uint32_t public_share_len,
                                   uint8_t leader_config_id, const uint8_t* d_leader_enc,
                                   uint32_t leader_enc_len, const uint8_t* d_leader_ct,
                                   const uint32_t* d_leader_ct_len, uint32_t leader_ct_stride,
                                   uint8_t helper_config_id, const uint8_t* d_helper_enc,
                                   uint32_t helper_enc_len, const uint8_t* d_helper_ct,
                                   const uint32_t* d_helper_ct_len, uint32_t helper_ct_stride,
                                   const uint8_t* d_skip, uint8_t* d_out, uint32_t out_stride,
                                   uint32_t* d_out_len, void* stream);
int64_t janus_dap_report_encode_host(uint32_t n, const uint8_t* report_ids, const uint64_t* times,
                                     const uint8_t* public_shares, uint32_t public_share_len,
                                     uint8_t leader_config_id, const uint8_t* leader_enc,
                                     uint32_t leader_enc_len, const uint8_t* leader_ct,
                                     const uint32_t* leader_ct_len, uint32_t leader_ct_stride,
                                     uint8_t helper_config_id, const uint8_t* helper_enc,
                                     uint32_t helper_enc_len, const uint8_t* helper_ct,
                                     const uint32_t* helper_ct_len, uint32_t helper_ct_stride,
                                     const uint8_t* skip, uint8_t* out, uint32_t out_stride,
                                     uint32_t* out_len);

/* ---- Leader side: the upload body, decoded ----------------------------------------------------
 * The inverse of janus_dap_report_encode_*, for the leader's upload handler
 * (`Report::get_decoded`, aggregator.rs handle_upload_generic): the same row form as input,
 * reports[n][report_stride] with report_len[n], one uploaded body per row.  Per report:
 *   report_ids[n][16], times[n], leader_config_ids[n], helper_config_ids[n],
 *   fields[n][JANUS_DAP_REPORT_FIELDS] (u32): byte offset within the row and length of the public
 *     share, and of `enc` and the payload of the leader's and the helper's HpkeCiphertext, at the
 *     JANUS_DAP_REPORT_* indices -- the large fields stay in place in the row,
 *   the helper's ciphertext copied out as the rows janus_dap_agg_init_req_encode_* reads:
 *     helper_enc[n][helper_enc_len], helper_ct[n][helper_ct_stride] with helper_ct_len[n] (bytes
 *     of a row past its payload are zero).  A helper `enc` of another length than helper_enc_len,
 *     or a payload above helper_ct_stride, gives helper_ct_len 0 and zero rows (the helper fails
 *     that report's HPKE open); fields[] still holds the lengths found.
 *   malformed[n]: 1 when the Report does not decode -- a length prefix runs past report_len, bytes
 *     trail the second ciphertext, or report_len > report_stride.  Every output of such a report is
 *     zero.  A public share or `enc` of an unexpected length is not malformed here.
 * No byte past report_len or report_stride is read.  helper_enc_len above 0xFFFF, a report_stride
 * of 2^31 or more, or a missing buffer is JANUS_DAP_EARG.
 * Host form: needs no GPU; returns the number of reports that decoded, or JANUS_DAP_EARG.
 * Device form: runs on `stream` of the GPU that owns d_malformed without host synchronisation; the
 * calling thread's current device is left as it was. */
#define JANUS_DAP_REPORT_FIELDS 10
enum {
  JANUS_DAP_REPORT_PUBLIC_SHARE_OFF = 0,
  JANUS_DAP_REPORT_PUBLIC_SHARE_LEN = 1,
  JANUS_DAP_REPORT_LEADER_ENC_OFF = 2,
  JANUS_DAP_REPORT_LEADER_ENC_LEN = 3,
  JANUS_DAP_REPORT_LEADER_PAYLOAD_OFF = 4,
  JANUS_DAP_REPORT_LEADER_PAYLOAD_LEN = 5,
  JANUS_DAP_REPORT_HELPER_ENC_OFF = 6,
  JANUS_DAP_REPORT_HELPER_ENC_LEN = 7,
  JANUS_DAP_REPORT_HELPER_PAYLOAD_OFF = 8,
  JANUS_DAP_REPORT_HELPER_PAYLOAD_LEN = 9
};
int64_t janus_dap_report_decode_host(uint32_t n, const uint8_t* reports, uint32_t report_stride,
                                     const uint32_t* report_len, uint8_t* report_ids,
                                     uint64_t* times, uint32_t* fields, uint8_t* leader_config_ids,
                                     uint8_t* helper_config_ids, uint8_t* helper_enc,
                                     uint32_t helper_enc_len, uint8_t* helper_ct,
                                     uint32_t* helper_ct_len, uint32_t helper_ct_stride,
                                     uint8_t* malformed);
int janus_dap_report_decode_device(uint32_t n, const uint8_t* d_reports, uint32_t report_stride,
                                   const uint32_t* d_report_len, uint8_t* d_report_ids,
                                   uint64_t* d_times, uint32_t* d_fields,
                                   uint8_t* d_leader_config_ids, uint8_t* d_helper_config_ids,
                                   uint8_t* d_helper_enc, uint32_t helper_enc_len,
                                   uint8_t* d_helper_ct, uint32_t* d_helper_ct_len,
                                   uint32_t helper_ct_stride, uint8_t* d_malformed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
