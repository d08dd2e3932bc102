/*
 * gck.h — C ABI of the MI355X batched permission-check engine (libgck.so).
 *
 * This is the drop-in boundary for gochugaru's check path. A Go caller binds
 * it through cgo; the Python host mirror (gochugaru_amd/engine.py) binds it
 * through ctypes. Signatures use plain pointers and sizes only.
 *
 * Reference interfaces replaced (authzed/gochugaru @ 2025-10-03):
 *   gck_check_bulk / gck_check_bulk_device
 *       replace the CheckBulkPermissions round-trip made by Client.Check
 *       (client/client.go:261-266) and consumed at client/client.go:271-283; transitively
 *       CheckOne/CheckAny/CheckAll/CheckIter (client/client.go:129-180).
 *   gck_load_schema
 *       consumes the schema text returned by Client.ReadSchema (client/client.go:416-422).
 *   gck_begin_snapshot / gck_add_tuples / gck_add_tuples_text / gck_load_csr / gck_commit_snapshot
 *   gck_save_snapshot / gck_load_snapshot_file (on-disk snapshot cache)
 *       consume the relationships streamed by Client.ExportRelationships at the schema's
 *       revision (client/client.go:472-499, rel.FromV1Proto rel/relationship.go:147-172).
 *   gck_intern
 *       replaces the per-item string handling of Client.Check's item loop
 *       (client/client.go:242-259) with batched string -> dense u32 interning.
 *   gck_apply_updates / gck_apply_updates_text (or gck_watch_stage + gck_watch_apply_staged)
 *       consume the rel.Update stream of Client.UpdatesSinceRevision (client/client.go:370-413,
 *       rel.UpdateFromV1Proto rel/relationship.go:296-301) and keep the snapshot current.
 *   gck_check_bulk_ctx / gck_check_bulk_device_ctx
 *       additionally take the check-time caveat contexts (CheckBulkPermissionsRequestItem.Context,
 *       client/client.go:257, from rel.Relationship.MustV1ProtoCaveat rel/relationship.go:174-188).
 *   gck_revision / gck_check_bulk's consistency argument
 *       honour consistency.Strategy (consistency/consistency.go:15-77) as sent in
 *       CheckBulkPermissionsRequest.Consistency (client/client.go:263).
 *
 *   gck_check_submit / gck_check_wait
 *       the same round-trip split in two, so that a caller keeps several CheckBulkPermissions
 *       batches in flight (Client.CheckIter's chunks, client/client.go:164-180, or concurrent
 *       Client.Check calls) and the device overlaps them.
 *   gck_set_head_revision
 *       the revision consistency.Full() (consistency/consistency.go:25-35) must reach: the
 *       ReadAt token of Client.ReadSchema (client/client.go:416-422) or a Watch checkpoint.
 *   gck_check_bulk_at / gck_check_wait_at
 *       the same calls, also returning the revision the batch was evaluated at: the response's
 *       CheckedAt token (CheckBulkPermissionsResponse.CheckedAt, read by consistency users of
 *       client/client.go:261-266).
 *   gck_check_bulk_uniform / gck_check_submit_uniform
 *       the common homogeneous request of Client.Check's item loop (client/client.go:241-259: one
 *       CheckBulkPermissionsRequestItem per relationship, all of one resource type, permission,
 *       subject type and subject relation) as one header and 8-byte (resource id, subject id)
 *       pairs, answered as a packed 2-bit Permissionship plane plus a sparse per-item error list.
 *   gck_check_bulk_shaped / gck_check_submit_shaped
 *       any request of that loop that mixes at most GCK_MAX_SHAPES shapes check by check: a table
 *       of headers, one table index byte and one id pair per check (9 bytes), answered the same way.
 *   gck_check_bulk_uniform_device / _shaped_device / _list_device and their gck_check_submit_* forms
 *       the same compact requests for a caller whose ids already live in device memory (a device-side
 *       candidate generator, a PyTorch pipeline): pairs, index bytes and id lists are read from, and
 *       the packed plane and the ascending error list written to, device buffers; nothing per check
 *       crosses PCIe.
 *   gck_filter_list_device / gck_filter_submit_list_device
 *       the list device request with its last step on the device too: the checks whose Permissionship
 *       a mask selects, compacted by a kernel into device arrays of ids, positions and
 *       Permissionships in the caller's order, and their number.
 *   gck_filter_cross_device / gck_filter_submit_cross_device
 *       the cross device request likewise: each subject's surviving resources, optionally the first K
 *       of them, compacted by kernels into a CSR (row offsets, ids, columns, Permissionships).
 *   gck_filter_cross_cols_device / gck_filter_submit_cross_cols_device
 *       its mirror: each resource's surviving subjects, optionally the first K of them, as a CSR by
 *       resource (column offsets, ids, rows, Permissionships).
 *   gck_recheck_list_device / gck_recheck_cross_device, their gck_recheck_submit_* forms and
 *   gck_diff_planes_device / gck_diff_cross_planes_device
 *       the list and cross device requests evaluated again after a Watch batch and compared on the
 *       device with the caller's previous plane: the ordered records of the checks that changed.
 *
 * Ownership: all inputs and outputs are caller-allocated; the engine never retains a caller
 * pointer after a call returns, except that gck_check_submit keeps the output pointers (and, for
 * device batches or host items in gck_host_alloc memory, the item pointer) until the matching
 * gck_check_wait. Return value: GCK_OK (0)
 * or a negative GCK_E_* status; the message is available from gck_last_error() (thread-local; the
 * message of the thread's last failure — a later success leaves it, as errno).
 * Threading: gck_check_bulk*, gck_check_submit / gck_check_wait and the lookups may be called
 * concurrently from any number of threads: each batch in flight runs on its own pooled
 * workspace and HIP stream (gck_config.workspaces of them; a call waits for a free one).
 * Schema, snapshot and Watch calls are exclusive: they first finish every batch in flight,
 * which keeps the results of the snapshot it was submitted against.
 */
#ifndef GCK_H
#define GCK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCK_ABI_VERSION 13

/* ---- status codes ------------------------------------------------------------------- */
#define GCK_OK 0
#define GCK_E_INVALID_ARGUMENT (-1) /* gRPC InvalidArgument */
#define GCK_E_SCHEMA (-2)           /* schema text failed to parse/validate */
#define GCK_E_NOT_FOUND (-3)        /* unknown type/relation name in a lookup */
#define GCK_E_DEVICE (-4)           /* HIP failure: map to gRPC Unavailable (caller retries) */
#define GCK_E_CAPACITY (-5)         /* a device workspace limit was exceeded */
#define GCK_E_STATE (-6)            /* wrong call order (no schema / no snapshot) */
#define GCK_E_REVISION (-7)         /* consistency requirement not satisfiable locally */
#define GCK_E_NO_DEVICE (-8)        /* no HIP device / HIP runtime unavailable */
#define GCK_E_REVISION_GONE (-9)    /* consistency.Snapshot at a revision the snapshot has moved past:
                                       permanent (SpiceDB: FailedPrecondition), not retriable */

/* ---- Permissionship (authzed v1 CheckPermissionResponse.Permissionship) --------------- */
#define GCK_PERM_UNSPECIFIED 0
#define GCK_PERM_NO 1
#define GCK_PERM_HAS 2
#define GCK_PERM_CONDITIONAL 3

/* ---- per-item errors (CheckBulkPermissionsPair.Error) --------------------------------- */
#define GCK_ITEM_OK 0
#define GCK_ITEM_ERR_MAX_DEPTH 1                /* dispatch depth budget exhausted */
#define GCK_ITEM_ERR_UNKNOWN_PERMISSION 2       /* permission not defined on the type */
#define GCK_ITEM_ERR_UNKNOWN_TYPE 3             /* resource or subject type not defined */
#define GCK_ITEM_ERR_UNKNOWN_SUBJECT_RELATION 4 /* subject relation not defined */
#define GCK_ITEM_ERR_WILDCARD_SUBJECT 5         /* subject id "*" is not checkable */
#define GCK_ITEM_ERR_CAVEAT_EVAL 6              /* a caveat on the check's walk failed to evaluate
                                                   under its context (a type error, a bad value) */

/* ---- special ids ---------------------------------------------------------------------- */
#define GCK_ELLIPSIS 0xFFFFu          /* subject relation "..." (a concrete object) */
#define GCK_ID_WILDCARD 0xFFFFFFFFu   /* subject id "*" */
#define GCK_ID_ABSENT 0xFFFFFFFEu     /* an id that is not in the snapshot */
#define GCK_TYPE_INVALID 0xFFFFu

/* ---- consistency requirement (consistency.Strategy) ------------------------------------ */
#define GCK_CONSISTENCY_MIN_LATENCY 0
#define GCK_CONSISTENCY_FULL 1
#define GCK_CONSISTENCY_AT_LEAST 2
#define GCK_CONSISTENCY_SNAPSHOT 3

/* ---- flags ---------------------------------------------------------------------------- */
#define GCK_INTERN_CREATE 1u     /* gck_intern: create ids for unseen strings */
#define GCK_MEM_DEVICE 1u        /* gck_load_csr: pointers are device memory */
#define GCK_FLAG_PROFILE 1u      /* gck_config.flags: time every kernel with HIP events */
#define GCK_FLAG_NO_BUNDLE 2u    /* gck_config.flags: grid-wide level-synchronous path only */
#define GCK_FLAG_NO_MHASH 4u     /* gck_config.flags: no hashed membership index (binary search) */
#define GCK_FLAG_NO_GIANT 8u     /* gck_config.flags: deferred checks skip the workgroup-bundle stage */
#define GCK_FLAG_NO_BIDIR 16u    /* gck_config.flags: forward-only search (no bidirectional checks) */
#define GCK_FLAG_NO_CLOSURE 32u  /* gck_config.flags: no closure-join stage (nested-group checks take
                                    the bundle search) */
#define GCK_FLAG_NO_SLOTS 128u  /* gck_config.flags: no per-user / per-resource slots for the
                                   closure join (saves ~128 B per user of HBM; slower) */
#define GCK_FLAG_NO_LABELS 256u  /* gck_config.flags: no label-join stage (hub hierarchy labels and
                                    flattened resource slots; labels.inc) */
#define GCK_FLAG_RESIDENT 512u  /* gck_config.flags: nested-group (closure-join) batches dispatched on the
                                    engine's queues go to one resident launch per engine, whose
                                    workgroups take 128-check chunks of the posted requests, instead of
                                    a dispatch each (small requests: a 64K request sharded over GPUs) */
#define GCK_FLAG_LAZY_CAVEATS 64u /* gck_config.flags: always evaluate check-time caveat contexts
                                     lazily (only the pairs a walk meets; by default a call whose
                                     partial instances x distinct contexts is small evaluates them all) */
#define GCK_FLAG_BIG_MHASH 1024u  /* gck_config.flags: build hashed membership indexes above 4 GB too
                                     (by default a larger one is not built: the one-round joins never
                                     read it, and the checks they leave binary-search the row) */

typedef struct gck_engine gck_engine;

typedef struct gck_config {
  int32_t device;              /* HIP device ordinal */
  uint32_t max_depth;          /* dispatch depth budget; 0 = 50 (SpiceDB default) */
  uint32_t max_batch;          /* checks per device launch sequence; 0 = 65536 */
  uint32_t flags;              /* GCK_FLAG_* */
  uint64_t visited_capacity;   /* slots of the per-batch visited hash (power of 2); 0 = auto */
  uint64_t frontier_capacity;  /* entries per frontier buffer; 0 = auto */
  uint64_t segment_capacity;   /* row segments per level; 0 = auto */
  uint64_t query_capacity;     /* queries per batch (checks + sub-queries of joins); 0 = auto */
  uint32_t bundle_checks;      /* checks per wavefront bundle (1..48); 0 = 32 */
  uint32_t bundle_frontier;    /* frontier entries per wavefront; 0 = 4096 */
  uint32_t bundle_visited;     /* visited slots per wavefront (power of 2); 0 = 16384 */
  uint32_t bundle_waves_per_cu;/* resident wavefronts per CU for the bundle kernel; 0 = 8 */
  uint32_t bundle_budget;      /* entries one check may push in a wavefront bundle before it is
                                  handed to a 16-wave workgroup; 0 = 1024 */
  uint32_t giant_frontier;     /* frontier entries per 16-wave workgroup bundle; 0 = 65536 */
  uint32_t giant_visited;      /* visited slots per workgroup bundle (power of 2); 0 = 262144 */
  uint32_t giant_slots;        /* resident workgroup bundles; 0 = one per CU */
  uint32_t bidir_both;         /* bidirectional checks expand both sides while their two
                                  frontiers hold at most this many entries; 0 = 64 */
  uint32_t workspaces;         /* check batches in flight at once (concurrent callers and
                                  submitted batches), one device workspace each; 0 = 4. A
                                  submit waits for a free workspace: one thread must keep at
                                  most this many batches outstanding. Config 4 peaks at ~16
                                  in flight */
} gck_config;

/* One check item, interned: CheckBulkPermissionsRequestItem (client/client.go:244-258). */
typedef struct gck_item {
  uint16_t resource_type;
  uint16_t permission;         /* global relation id (gck_relation_id) */
  uint32_t resource_id;
  uint16_t subject_type;
  uint16_t subject_relation;   /* GCK_ELLIPSIS for a concrete object */
  uint32_t subject_id;
  uint32_t context_slot;       /* 0 = no check-time caveat context; k = contexts[k-1] of the
                                  gck_check_bulk*_ctx call */
} gck_item;                    /* 20 bytes */

/* One relationship, interned: rel.Relationship (rel/relationship.go:28-38). */
typedef struct gck_tuple {
  uint16_t resource_type;
  uint16_t relation;           /* global relation id */
  uint32_t resource_id;
  uint16_t subject_type;
  uint16_t subject_relation;   /* GCK_ELLIPSIS or a relation id of subject_type */
  uint32_t subject_id;         /* GCK_ID_WILDCARD for "type:*" */
  uint32_t caveat;             /* caveat instance id from gck_add_caveat_instance; 0 = none */
  int64_t expires_at_us;       /* unix microseconds; 0 = never */
} gck_tuple;                   /* 32 bytes */

/* One Watch update: rel.Update (rel/relationship.go:291-301), operation = rel.UpdateType. */
#define GCK_UPDATE_CREATE 1u   /* rel.UpdateCreate (applied as an upsert) */
#define GCK_UPDATE_DELETE 2u   /* rel.UpdateDelete */
#define GCK_UPDATE_TOUCH 3u    /* rel.UpdateTouch */
typedef struct gck_update {
  uint32_t op;                 /* GCK_UPDATE_* */
  uint32_t reserved;
  gck_tuple tuple;
} gck_update;                  /* 40 bytes */

typedef struct gck_consistency {
  int32_t requirement;         /* GCK_CONSISTENCY_* */
  uint32_t reserved;
  uint64_t revision;           /* AT_LEAST / SNAPSHOT token, decoded */
} gck_consistency;

typedef struct gck_stats {
  uint64_t batches;
  uint64_t levels;             /* BFS levels executed: grid-wide levels + every bundle's levels */
  uint64_t entries_expanded;   /* (query, object, node) entries expanded */
  uint64_t row_lookups;        /* CSR rows opened (each = one 8-B offset pair) */
  uint64_t membership_probes;  /* 4-B neighbour reads by membership binary searches */
  uint64_t edges_enumerated;   /* 4-B neighbour reads by userset/arrow enumeration */
  uint64_t ext_edges;          /* caveated/expiring edges read (+4 B caveat id +8 B expiry) */
  uint64_t queries;            /* queries allocated (checks + join operands) */
  uint64_t joins;              /* intersection/exclusion/all() joins spawned */
  uint64_t retries;            /* batch splits after a workspace overflow */
  double kernel_ms;            /* GCK_FLAG_PROFILE: device time of the last call's batches that were
                                  timed (HIP events around stage A on every 4th batch of a workspace) */
  double expand_ms;            /* GCK_FLAG_PROFILE: summed k_expand time (all batches) */
  double edges_ms;             /* GCK_FLAG_PROFILE: summed k_edges time */
  double resolve_ms;           /* GCK_FLAG_PROFILE: summed k_resolve time */
  uint64_t expand_launches;    /* GCK_FLAG_PROFILE: k_expand launches timed */
  uint64_t edges_launches;     /* GCK_FLAG_PROFILE: k_edges launches timed */
  double bundle_ms;            /* GCK_FLAG_PROFILE: summed stage-A time (closure join and/or wave
                                  bundles) of the timed batches (every 4th of a workspace) */
  uint64_t bundle_launches;    /* GCK_FLAG_PROFILE: batches whose stage A was timed */
  uint64_t deferred;           /* checks handed from wavefront bundles to workgroup bundles */
  double giant_ms;             /* GCK_FLAG_PROFILE: summed workgroup-bundle kernel time */
  uint64_t deferred_wide;      /* checks handed from workgroup bundles to the grid-wide path */
  uint64_t bidir_checks;       /* checks evaluated bidirectionally (forward + reverse frontier) */
  uint64_t bundles;            /* check bundles run by the bundle kernels (`levels` also sums
                                  their BFS levels) */
  uint64_t closure_checks;     /* checks answered by the closure-join stage (nested groups) */
  uint64_t caveat_evals;       /* (caveat instance, check context) pairs evaluated on the host */
  uint64_t caveat_passes;      /* extra batch passes after lazily evaluated caveat pairs */
  uint64_t slot_checks;        /* checks the closure join decided from their user / resource slots
                                  alone (one read each) */
  uint64_t label_checks;       /* of closure_checks: those the label join (labels.inc k_label_join,
                                  or its partitioned form) answered */
  uint64_t aql_batches;        /* batches whose join the engine dispatched into its own HSA queue
                                  (engine-stream device batches, aql.inc) instead of launching it
                                  through HIP */
  uint64_t resident_batches;   /* batches the resident join took (GCK_FLAG_RESIDENT) */
} gck_stats;

/* ---- lifecycle ------------------------------------------------------------------------ */
int gck_abi_version(void);
const char* gck_last_error(void);
int gck_create(const gck_config* cfg, gck_engine** out);
void gck_destroy(gck_engine* e);

/* ---- schema (Client.ReadSchema text, client/client.go:416-422) ------------------------ */
int gck_load_schema(gck_engine* e, const char* text, size_t len);
int gck_type_id(gck_engine* e, const char* name, size_t len, uint16_t* out);
int gck_relation_id(gck_engine* e, uint16_t type, const char* name, size_t len, uint16_t* out);
int gck_type_count(gck_engine* e, uint32_t* out);
int gck_relation_count(gck_engine* e, uint32_t* out);

/* ---- interning (Client.Check item loop, client/client.go:242-259) --------------------- */
int gck_intern(gck_engine* e, uint16_t type, const char* const* ids, const uint32_t* lens,
               size_t n, uint32_t flags, uint32_t* out_ids);
int gck_object_count(gck_engine* e, uint16_t type, uint32_t* out);
/* Declares ids [0, n) of `type` as existing (anonymous objects for bulk CSR ingest). */
int gck_reserve_objects(gck_engine* e, uint16_t type, uint32_t n);
int gck_object_name(gck_engine* e, uint16_t type, uint32_t id, char* buf, size_t cap,
                    size_t* out_len);

/* ---- caveats (rel.Relationship.CaveatName/CaveatContext) ------------------------------ */
/* A caveat name with its stored context (a JSON object; "" = none). Identical (name, context)
 * pairs return the same id. Errors: GCK_E_INVALID_ARGUMENT for an unknown caveat, malformed
 * JSON, or a stored context on which the expression fails to evaluate. */
int gck_add_caveat_instance(gck_engine* e, const char* name, size_t name_len,
                            const char* context_json, size_t json_len, uint32_t* out_id);

/* The host CEL evaluator on its own: caveat `name` over the stored context merged with the
 * check context (stored values take precedence). *out = 0 false, 1 true, 2 partial (a
 * parameter is missing: CONDITIONAL). GCK_E_NOT_FOUND for an unknown caveat. */
int gck_evaluate_caveat(gck_engine* e, const char* name, size_t name_len, const char* stored_json,
                        size_t stored_len, const char* context_json, size_t context_len, uint8_t* out);

/* ---- snapshot ingest (Client.ExportRelationships, client/client.go:472-499) ----------- */
int gck_begin_snapshot(gck_engine* e, uint64_t revision);
int gck_add_tuples(gck_engine* e, const gck_tuple* tuples, size_t n);
/* Canonical rel.Relationship.String lines (rel/relationship.go:51-90), '\n'-separated. */
int gck_add_tuples_text(gck_engine* e, const char* text, size_t len);
/* Prebuilt CSR for one (relation, subject kind): rows sorted ascending, no duplicates,
 * plain edges only (no caveat/expiration). n_rows = object count of the relation's type. */
int gck_load_csr(gck_engine* e, uint16_t relation, uint16_t subject_type,
                 uint16_t subject_relation, uint32_t n_rows, const uint32_t* offsets,
                 const uint32_t* neighbours, uint64_t n_edges, uint32_t mem_flags);
int gck_commit_snapshot(gck_engine* e);
/* On-disk snapshot cache, in place of re-reading the snapshot through
 * Client.ExportRelationships (client/client.go:472-499) and re-interning it: save writes the
 * committed snapshot (interner, caveat instances, base CSRs, revision) keyed by the schema
 * text; load (same schema text, no staging in progress) replaces the committed snapshot and
 * rebuilds the derived device indexes. GCK_E_SCHEMA when the file was saved under another
 * schema; GCK_E_STATE to save a partitioned engine or with nothing committed. */
int gck_save_snapshot(gck_engine* e, const char* path);
int gck_load_snapshot_file(gck_engine* e, const char* path);
int gck_revision(gck_engine* e, uint64_t* out);
/* The source's head revision, for consistency.Full(): a Full check (or lookup) returns
 * GCK_E_REVISION — gRPC Unavailable, which the client retries — until the applied revision
 * (gck_commit_snapshot / gck_apply_updates) reaches it. 0 (the default) = the local snapshot is
 * the head. The head only moves forward. */
int gck_set_head_revision(gck_engine* e, uint64_t revision);
int gck_tuple_count(gck_engine* e, uint64_t* out);
/* Bytes resident in HBM for the snapshot (CSR + tables). */
int gck_device_bytes(gck_engine* e, uint64_t* out);

/* ---- Watch (Client.UpdatesSinceRevision, client/client.go:370-413) ------------------- */
/* Applies one batch of updates (a Watch response, in stream order) to the committed snapshot
 * and moves it to `revision` (the response's ChangesThrough token, decoded), which must be
 * newer than the current one; an empty batch may also re-state the current revision. The merge
 * runs on the device. Errors: GCK_E_REVISION (stale revision), GCK_E_INVALID_ARGUMENT (unknown
 * operation / relationship the schema rejects; nothing applied), GCK_E_STATE (no snapshot).
 * A device failure during the merge leaves no snapshot (GCK_E_STATE until the next commit). */
int gck_apply_updates(gck_engine* e, uint64_t revision, const gck_update* updates, size_t n);
/* Text form: one "<OP> <relationship>" per line, OP = CREATE | TOUCH | DELETE and the
 * relationship in rel.Relationship.String form (rel/relationship.go:51-90). */
int gck_apply_updates_text(gck_engine* e, uint64_t revision, const char* text, size_t len);
/* Pipelined Watch: a consumer that has the next batch while it applies the previous one stages it
 * — gck_watch_stage returns at once and an engine thread validates and groups the batch meanwhile
 * — then applies it with gck_watch_apply_staged, in stream order, which waits for the grouping and
 * applies as gck_apply_updates does (same errors; a batch the staging rejected, or staged before a
 * schema / snapshot-file / partition change, is grouped again there and its error reported).
 * `updates` must stay valid and unchanged until the ticket is applied or discarded. Up to 4
 * batches may be staged at once (GCK_E_CAPACITY beyond); a ticket is used once. */
int gck_watch_stage(gck_engine* e, const gck_update* updates, size_t n, uint64_t* ticket);
int gck_watch_apply_staged(gck_engine* e, uint64_t revision, uint64_t ticket);
int gck_watch_discard(gck_engine* e, uint64_t ticket);

/* ---- checks (CheckBulkPermissions, client/client.go:261-283) -------------------------- */
/* Host buffers: items[n] in, out_perm[n] (GCK_PERM_*), out_err[n] (GCK_ITEM_*) out.
 * `now_us` = the evaluation time for expiring relationships (unix microseconds; 0 = wall
 * clock). Results are in request order. Caveats are evaluated with the stored context only;
 * one that depends on a missing parameter makes its path CONDITIONAL. */
int gck_check_bulk(gck_engine* e, const gck_consistency* cs, const gck_item* items, size_t n,
                   int64_t now_us, uint8_t* out_perm, int32_t* out_err);
/* Same, with check-time caveat contexts: contexts[k] (JSON object text, context_lens[k] bytes)
 * is the context of every item whose context_slot is k + 1. A caveat is evaluated over its
 * stored context merged with the item's context (stored values take precedence): true = the
 * relationship counts, false = it does not, missing parameter = CONDITIONAL. Only the
 * (caveat instance, context) pairs the checks' walks meet are evaluated once the product of
 * partial instances and distinct contexts is large (the batch then runs again with their
 * outcomes); a pair that fails to evaluate gives the items whose walk met it
 * GCK_ITEM_ERR_CAVEAT_EVAL and nothing else.
 * Errors: GCK_E_INVALID_ARGUMENT (a context_slot > n_contexts, malformed JSON). */
int gck_check_bulk_ctx(gck_engine* e, const gck_consistency* cs, const gck_item* items, size_t n,
                       const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                       int64_t now_us, uint8_t* out_perm, int32_t* out_err);
/* Device-resident buffers on the engine's device. `stream` is the hipStream_t the caller
 * produced the items on and will read the results on; NULL is HIP's default (null) stream, as
 * for any HIP launch, so work the caller queued there (e.g. PyTorch's default stream) is
 * ordered before the check. Returns after the results are written (stream synchronised). */
int gck_check_bulk_device(gck_engine* e, const gck_item* d_items, size_t n, int64_t now_us,
                          uint8_t* d_out_perm, int32_t* d_out_err, void* stream);
/* Device buffers with host-side check contexts (as gck_check_bulk_ctx; a device item's
 * context_slot beyond n_contexts counts as no context). */
int gck_check_bulk_device_ctx(gck_engine* e, const gck_item* d_items, size_t n,
                              const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                              int64_t now_us, uint8_t* d_out_perm, int32_t* d_out_err, void* stream);
/* Asynchronous batches: gck_check_submit starts one batch of n <= max_batch items and returns at
 * once with a handle; gck_check_wait(handle) completes it (results written, handle consumed).
 * Every submitted batch must be waited for exactly once. GCK_SUBMIT_DEVICE: items / out_perm /
 * out_err are device buffers ordered on `stream` (as gck_check_bulk_device_ctx); otherwise they
 * are host buffers (the outputs are written by the wait; pageable items are staged before the
 * call returns, while items in gck_host_alloc memory are read by DMA as the batch runs and must
 * stay unchanged until gck_check_wait returns). Consistency is checked at submit; the batch sees the snapshot current at submit, even if
 * a Watch batch is applied before the wait. GCK_SUBMIT_DEVICE | GCK_SUBMIT_ENGINE_STREAM: device
 * buffers, but the batch runs on the stream of the workspace it holds (created by the engine, one
 * per workspace, so that batches in flight sit on distinct hardware queues) and `stream` is
 * ignored: the items must be complete when the call is made, and the results are complete when
 * gck_check_wait returns. */
typedef struct gck_batch gck_batch;
#define GCK_SUBMIT_DEVICE 1u
#define GCK_SUBMIT_ENGINE_STREAM 2u
int gck_check_submit(gck_engine* e, const gck_consistency* cs, const gck_item* items, size_t n,
                     const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                     int64_t now_us, uint8_t* out_perm, int32_t* out_err, uint32_t flags, void* stream,
                     gck_batch** out);
int gck_check_wait(gck_engine* e, gck_batch* batch);
/* Pinned host memory for request / result buffers: a host batch (gck_check_bulk*,
 * gck_check_submit) whose items or results lie in such a buffer is copied over PCIe by DMA
 * directly, skipping the engine's own staging copy (a submitted batch then reads its items there
 * until gck_check_wait). Freed with gck_host_free (or gck_destroy). */
int gck_host_alloc(gck_engine* e, size_t bytes, void** out);
int gck_host_free(gck_engine* e, void* p);
int gck_last_stats(gck_engine* e, gck_stats* out);
int gck_reset_stats(gck_engine* e);
/* Turns GCK_FLAG_PROFILE on or off for the batches submitted from now on (a timed batch brackets
 * its stage A with the kernel's own start/stop events, every 4th batch of a workspace). */
int gck_set_profile(gck_engine* e, uint32_t on);

/* The revision a check was evaluated at (ABI 13). gck_check_bulk_at is gck_check_bulk_ctx that
 * also writes the revision of the snapshot the batch ran on to *out_revision (may be NULL): the
 * response's CheckedAt. A submitted batch runs on the snapshot current at its submit, and
 * gck_check_wait_at reports that revision — not the one current at the wait, which a Watch batch
 * applied in between may have moved. */
int gck_check_bulk_at(gck_engine* e, const gck_consistency* cs, const gck_item* items, size_t n,
                      const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                      int64_t now_us, uint8_t* out_perm, int32_t* out_err, uint64_t* out_revision);
int gck_check_wait_at(gck_engine* e, gck_batch* batch, uint64_t* out_revision);

/* ---- uniform requests (ABI 13) -------------------------------------------------------
 * A request whose items share (resource type, permission, subject type, subject relation, context
 * slot) — what Client.Check sends for relationships of one shape (client/client.go:241-259) —
 * travels as one header and n (resource id, subject id) pairs: 8 bytes per check over PCIe
 * instead of 20. Results come back packed: check k's Permissionship (GCK_PERM_*) in bits
 * 2(k mod 32) .. 2(k mod 32) + 1 of out_packed[k / 32] (ceil(n / 32) words; GCK_PERM_UNSPECIFIED
 * for a check with an error), and the checks with an error as (index, GCK_ITEM_*) records in
 * ascending index order: *out_n_errs = how many checks have one, the first min(that, err_cap) of
 * them are written to out_errs. Semantics, consistency and request errors are gck_check_bulk_at's;
 * a context_slot beyond n_contexts is GCK_E_INVALID_ARGUMENT. Pairs and results in gck_host_alloc
 * memory are read and written in place by the kernels. */
typedef struct gck_uniform {
  uint16_t resource_type;
  uint16_t permission;         /* global relation id (gck_relation_id) */
  uint16_t subject_type;
  uint16_t subject_relation;   /* GCK_ELLIPSIS for a concrete object */
  uint32_t context_slot;       /* as gck_item.context_slot, for every pair */
  uint32_t reserved;           /* 0 */
} gck_uniform;                 /* 16 bytes */
typedef struct gck_item_error {
  uint32_t index;              /* the check's position in the request */
  int32_t code;                /* GCK_ITEM_* (never GCK_ITEM_OK) */
} gck_item_error;
int gck_check_bulk_uniform(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, const uint32_t* pairs,
                           size_t n, const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                           int64_t now_us, uint64_t* out_packed, gck_item_error* out_errs, size_t err_cap,
                           size_t* out_n_errs, uint64_t* out_revision);
/* The same as an asynchronous batch (n <= max_batch; host buffers): completed by gck_check_wait or
 * gck_check_wait_at, which write out_packed, out_errs and *out_n_errs. `pairs`, `hdr` and the
 * outputs must stay valid until the wait returns. */
int gck_check_submit_uniform(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, const uint32_t* pairs,
                             size_t n, const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                             int64_t now_us, uint64_t* out_packed, gck_item_error* out_errs, size_t err_cap,
                             size_t* out_n_errs, gck_batch** out);

/* ---- shaped requests (ABI 13, additive) ----------------------------------------------
 * A request that mixes permissions, resource types, subject kinds or context slots check by check
 * — what Client.Check sends for arbitrary relationships — travels as a small table of shapes
 * (gck_uniform headers; 1..GCK_MAX_SHAPES entries, which may repeat), one table index byte per
 * check and the (resource id, subject id) pairs: 9 bytes per check in and 1/4 byte out, whatever
 * the order of the checks. Check k is (shapes[shape_of[k]], pairs[2k], pairs[2k + 1]). Results are
 * the uniform call's: the packed 2-bit words and the ascending (index, GCK_ITEM_*) error records;
 * semantics, consistency and request errors are gck_check_bulk_at's. GCK_E_INVALID_ARGUMENT for
 * n_shapes outside 1..GCK_MAX_SHAPES, a shape whose context_slot exceeds n_contexts or whose
 * `reserved` is not 0, null buffers, and a shape_of[k] >= n_shapes (the message names the smallest
 * such k of the request; out_packed may then be partly written).
 * Lifetimes: `shapes` is copied by the call and need not outlive it (the submit call included);
 * `shape_of`, `pairs` and the outputs follow the uniform rule — valid until the synchronous call
 * returns, or until the wait of a submitted batch returns. shape_of, pairs and out_packed in
 * gck_host_alloc memory are read and written in place by the kernels. */
#define GCK_MAX_SHAPES 64
int gck_check_bulk_shaped(gck_engine* e, const gck_consistency* cs, const gck_uniform* shapes, size_t n_shapes,
                          const uint8_t* shape_of, const uint32_t* pairs, size_t n, const char* const* contexts,
                          const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                          gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, uint64_t* out_revision);
/* The same as an asynchronous batch (n <= max_batch): completed by gck_check_wait or
 * gck_check_wait_at, which write out_packed, out_errs and *out_n_errs (and report a bad shape
 * index found by the kernel). */
int gck_check_submit_shaped(gck_engine* e, const gck_consistency* cs, const gck_uniform* shapes, size_t n_shapes,
                            const uint8_t* shape_of, const uint32_t* pairs, size_t n, const char* const* contexts,
                            const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                            gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, gck_batch** out);
/* Since the engine was created: out[0] = shaped requests (chunks of max_batch) whose join read the
 * request in place, out[1] = those expanded to items on the host (check contexts, profiling, no
 * one-round join). */
int gck_shaped_stats(gck_engine* e, uint64_t out[2]);

/* ---- cross requests (ABI 13, additive) -----------------------------------------------
 * Every subject of one list against every resource of another, all of one shape — "which of
 * these documents may this user see", an access review of a team against a folder — travels as
 * one header and the two id lists: 4 (S + R) bytes in for S * R checks. Check (s, r) is
 * (hdr, resources[r], subjects[s]); semantics, consistency and request errors are
 * gck_check_bulk_at's. Ids are not deduplicated; a list may repeat an id.
 * Results: rows by subject, each row padded to whole words, stride = ceil(R / 32) words — the
 * Permissionship of (s, r) is bits 2 (r % 32) .. +1 of out_packed[s * stride + r / 32]; padding
 * bits are 0 and every one of the S * stride words is written. The error records are the uniform
 * call's (index, GCK_ITEM_*) with index = s * R + r, ascending, under the same err_cap / *out_n_errs
 * protocol. GCK_E_INVALID_ARGUMENT for null buffers with S * R > 0, a header whose `reserved` is
 * not 0 or whose context_slot exceeds n_contexts, and S * R >= 2^32. S == 0 or R == 0 is an empty
 * request that succeeds.
 * Lifetimes: both lists are copied by the call and need not outlive it (the submit call
 * included); the outputs follow the uniform rule. */
#define GCK_CROSS_IDS 2048 /* ids (subjects + resources) a tile holds in the workspace's id block */
int gck_check_bulk_cross(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, const uint32_t* subjects,
                         size_t n_subjects, const uint32_t* resources, size_t n_resources, const char* const* contexts,
                         const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                         gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, uint64_t* out_revision);
/* The same as an asynchronous batch of one tile — gck_cross_tile(S, R, max_batch) must return the
 * whole request, else GCK_E_INVALID_ARGUMENT: completed by gck_check_wait or gck_check_wait_at,
 * which write out_packed, out_errs and *out_n_errs. */
int gck_check_submit_cross(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, const uint32_t* subjects,
                           size_t n_subjects, const uint32_t* resources, size_t n_resources,
                           const char* const* contexts, const size_t* context_lens, size_t n_contexts, int64_t now_us,
                           uint64_t* out_packed, gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs,
                           gck_batch** out);
/* Since the engine was created: out[0] = tiles whose join read the two lists in place, out[1] =
 * chunks of max_batch checks expanded to items on the host (check contexts, profiling, no
 * one-round join, GCK_AQL=0, or a thin request: gck_cross_tile returned 0). */
int gck_cross_stats(gck_engine* e, uint64_t out[2]);
/* The tiling rule (pure: no engine, no device; the engine itself calls it). Returns 1 with the
 * tile *rows x *cols (subjects x resources) an in-place request is cut into, left to right and
 * top to bottom with ragged last tiles, or 0 (*rows = *cols = 0) when the request is to be
 * expanded. A tile satisfies rows * 32 * ceil(cols / 32) <= max_batch, rows + cols <=
 * GCK_CROSS_IDS, cols % 32 == 0 or cols == R, rows <= S, cols <= R; among such tiles the one with
 * the most checks, the wider one on a tie. 0 when no tile exists (an empty list, max_batch < 32),
 * or when the request has more checks than the best tile and that tile holds fewer than
 * max_batch / 4: a thin request (one subject against 60,000 resources) would become dozens of
 * small dispatches. */
int gck_cross_tile(size_t n_subjects, size_t n_resources, size_t max_batch, uint32_t* rows, uint32_t* cols);

/* ---- list requests (ABI 13, additive) ------------------------------------------------
 * One fixed id against many ids of the other side, all of one shape — "which of these 60,000
 * documents may this user see", and its mirror, "which of these users may see this document":
 * one header, the fixed id, and 4 B per check — or nothing per check. `vary` says which side the
 * n ids are: GCK_VARY_RESOURCE (fixed_id is the subject id) or GCK_VARY_SUBJECT (fixed_id is the
 * resource id). Check i is (hdr, fixed_id, v_i) with
 *   - an id list: v_i = ids[i]; in gck_host_alloc memory the kernels read it in place, under the
 *     lifetime rule of a uniform request's `pairs` (a pageable list is staged as pageable pairs
 *     are); `first_id` is ignored;
 *   - a range: ids == NULL and v_i = first_id + i, the form of a sweep over a whole type. A range
 *     varies the resource id.
 * Semantics, consistency and request errors are gck_check_bulk_uniform's, ids included: they are
 * not deduplicated, may be GCK_ID_ABSENT or GCK_ID_WILDCARD where that call allows them, and an
 * id beyond the type's objects is answered as that call answers it (NO: the object has no
 * relationships). Results are the uniform call's too: the dense plane of ceil(n / 32) words
 * (padding bits 0, every word written), the ascending (index, GCK_ITEM_*) records under the same
 * err_cap / *out_n_errs protocol. GCK_E_INVALID_ARGUMENT also for a `vary` that is neither value,
 * a header whose `reserved` is not 0, a range with first_id + n > 2^32, and a range with
 * GCK_VARY_SUBJECT. n == 0 succeeds and writes nothing. */
#define GCK_VARY_RESOURCE 1u
#define GCK_VARY_SUBJECT 2u
int gck_check_bulk_list(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                        uint32_t vary, const uint32_t* ids, uint32_t first_id, size_t n, const char* const* contexts,
                        const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                        gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, uint64_t* out_revision);
/* The same as an asynchronous batch of one chunk (n <= max_batch): completed by gck_check_wait or
 * gck_check_wait_at, which write out_packed, out_errs and *out_n_errs. An id list in
 * gck_host_alloc memory must stay unchanged until the wait returns; any other list is copied by
 * the call. */
int gck_check_submit_list(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                          uint32_t vary, const uint32_t* ids, uint32_t first_id, size_t n, const char* const* contexts,
                          const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                          gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, gck_batch** out);
/* Since the engine was created: out[0] = chunks (of max_batch checks) whose join read the ids in
 * place or computed them from the range, out[1] = chunks expanded to items on the host (check
 * contexts, profiling, no one-round join, GCK_AQL=0). */
int gck_list_stats(gck_engine* e, uint64_t out[2]);

/* ---- compact requests over device buffers (ABI 13, additive) -------------------------
 * The uniform, shaped and list requests above for ids that live in device memory: d_pairs,
 * d_shape_of, d_ids, d_out_packed, d_out_errs and d_out_n_errs (a uint32_t) are device memory on the
 * engine's device; hdr, shapes (copied by the call), contexts and out_revision are host memory.
 * d_ids == NULL is the range form (first_id + i, GCK_VARY_RESOURCE only), which reads nothing.
 * Check k, the word layout (padding bits 0, every one of the ceil(n / 32) words written,
 * GCK_PERM_UNSPECIFIED for a check with an error) and the err_cap / count protocol are the host
 * calls': the (index, GCK_ITEM_*) records in ascending index order, the first min(count, err_cap)
 * written to d_out_errs, the count to *d_out_n_errs — always, 0 and n == 0 included, when the pointer
 * is not NULL. d_out_n_errs may be NULL; d_out_errs may be NULL when err_cap == 0. The list is
 * produced on the device: no per-check data crosses PCIe.
 * Ordering is gck_check_bulk_device's and gck_check_submit's: a synchronous call orders on `stream`
 * (NULL: the null stream) and returns with the results written; it chunks as the host forms do. A
 * submitted batch (n <= max_batch) with flags 0 runs on the caller's `stream`; with
 * GCK_SUBMIT_ENGINE_STREAM on the stream of its workspace: the inputs must be complete at the call
 * and the results are complete when gck_check_wait / gck_check_wait_at returns. GCK_SUBMIT_DEVICE is
 * accepted and implied. Buffers stay valid and unchanged until the synchronous call or the wait
 * returns. Consistency, request errors and the evaluated revision are the host calls'.
 * GCK_E_INVALID_ARGUMENT also for a d_pairs or d_out_packed that is not 8-byte aligned (the joins
 * load a pair as one 64-bit word), a d_ids, d_out_errs or d_out_n_errs that is not 4-byte aligned,
 * n >= 2^32 (nothing is launched for any of these), and a shape_of[k] >= n_shapes found on the
 * device, reported by the synchronous call or by the wait with the smallest such k of the request. */
int gck_check_bulk_uniform_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                                  const uint32_t* d_pairs, size_t n, const char* const* contexts,
                                  const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* d_out_packed,
                                  gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, void* stream,
                                  uint64_t* out_revision);
int gck_check_bulk_shaped_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* shapes, size_t n_shapes,
                                 const uint8_t* d_shape_of, const uint32_t* d_pairs, size_t n,
                                 const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                 int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                 uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision);
int gck_check_bulk_list_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                               uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                               const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                               int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                               uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision);
int gck_check_submit_uniform_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                                    const uint32_t* d_pairs, size_t n, const char* const* contexts,
                                    const size_t* context_lens, size_t n_contexts, int64_t now_us,
                                    uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                    uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out);
int gck_check_submit_shaped_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* shapes,
                                   size_t n_shapes, const uint8_t* d_shape_of, const uint32_t* d_pairs, size_t n,
                                   const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                   int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                   uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out);
int gck_check_submit_list_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                                 uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                                 const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                 int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                 uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out);
/* Since the engine was created: out[0] = chunks (of max_batch checks) of device requests whose join
 * read the request and wrote the words in place in device memory, out[1] = chunks expanded to items
 * on the device (check contexts, profiling, no one-round join, GCK_AQL=0, GCK_FLAG_NO_BUNDLE).
 * gck_shaped_stats, gck_list_stats and gck_cross_stats do not count device requests. A cross device
 * request (below) counts here too: out[0] its tiles read in place, out[1] its chunks expanded. */
int gck_device_compact_stats(gck_engine* e, uint64_t out[2]);

/* ---- cross requests over device buffers (ABI 13, additive) ---------------------------
 * gck_check_bulk_cross / gck_check_submit_cross for id lists that live in device memory — a batch of
 * user ids and a page of candidate ids as two tensors: d_subjects, d_resources, d_out_packed,
 * d_out_errs and d_out_n_errs (a uint32_t) are device memory on the engine's device. Check (s, r), the
 * row-padded plane (stride = ceil(R / 32) words, padding bits 0, every one of the S * stride words
 * written, an errored check 0) and the records (index = s * R + r, ascending) are the host cross
 * call's; the err_cap / *d_out_n_errs protocol, stream ordering, GCK_SUBMIT_ENGINE_STREAM,
 * consistency, the evaluated revision and buffer lifetimes are the device compact calls' above. Unlike
 * the host cross call the two lists are NOT copied: they stay valid and unchanged until the
 * synchronous call or the wait returns.
 * In place the request is cut into full-width tiles, gck_cross_tile_device(S, R, max_batch) subjects
 * by all R resources, band after band from the top: a tile's words are a contiguous run of the
 * caller's plane, which the join writes directly, after one small kernel has put the tile's ids into
 * the workspace's id block. A layout a caller may use to spare even that: one buffer of the R resource
 * ids, padding to a multiple of four words, then the S subject ids (d_subjects == d_resources +
 * ((R + 3) & ~3), in words) — when the request is one tile the join reads that buffer where it is.
 * Otherwise (check contexts, profiling, no one-round join, GCK_AQL=0, GCK_FLAG_NO_BUNDLE, or a 0 from
 * the tiling rule — R >= GCK_CROSS_IDS among them) the request is expanded to items on the device in
 * row-major chunks of max_batch checks.
 * GCK_E_INVALID_ARGUMENT, nothing launched, for everything the host cross call refuses (`reserved`,
 * the context slot, S * R >= 2^32, null lists with S * R > 0), a d_out_packed that is not 8-byte
 * aligned, and a d_subjects, d_resources, d_out_errs or d_out_n_errs that is not 4-byte aligned.
 * S == 0 or R == 0 succeeds and writes only the count word. The submit form takes a request that is
 * one device tile (gck_cross_tile_device returns S), else GCK_E_INVALID_ARGUMENT.
 * gck_device_compact_stats counts these requests' tiles and chunks; gck_cross_stats does not. */
int gck_check_bulk_cross_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                                const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                size_t n_contexts, int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                                size_t err_cap, uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision);
int gck_check_submit_cross_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                                  const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                  size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                  size_t n_contexts, int64_t now_us, uint64_t* d_out_packed,
                                  gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, uint32_t flags,
                                  void* stream, gck_batch** out);
/* The device tiling rule (pure, as gck_cross_tile): *rows = the subjects of a full-width tile,
 * min(S, max_batch / (32 * ceil(R / 32)), GCK_CROSS_IDS - R), and 1 returned; or 0 (*rows = 0: the
 * request is expanded) when that is 0, R >= GCK_CROSS_IDS, 32 * ceil(R / 32) > max_batch, or the
 * request has more checks than the tile and the tile holds fewer than max_batch / 4 (gck_cross_tile's
 * thin rule). */
int gck_cross_tile_device(size_t n_subjects, size_t n_resources, size_t max_batch, uint32_t* rows);

/* ---- filter requests (ABI 13, additive) ----------------------------------------------
 * gck_check_bulk_list_device / gck_check_submit_list_device with the last step done on the device
 * too: of the n checks of the list request, the survivors — their varying ids, their positions in
 * the request and their Permissionships — compacted by a kernel into the caller's device arrays, in
 * the caller's order. The check itself is the list device call's, unchanged: the id list or range,
 * `vary`, consistency, the chunking of the synchronous form, stream ordering, `flags`, lifetimes,
 * the error records and the request errors.
 * Check i survives iff it has no per-item error and (sel->mask >> perm_i) & 1. Survivors are written
 * in ascending i, an id as often as the list repeats it: the first min(total, cap) of them to each
 * output array that is not NULL, entries beyond that untouched. *d_out_n = the survivors of the whole
 * request — always written, for 0 survivors and for n == 0 too.
 * A check with an error never survives; it is reported through d_out_errs / *d_out_n_errs as the list
 * device call reports it. Unlike gck_lookup_resources_among, the device form does NOT fail the call
 * on a per-item error: the caller holds the count word and decides.
 * d_out_packed may be NULL: the plane then stays in a device buffer of the workspace (allocated with
 * it; no check allocates). When given, it is written exactly as gck_check_bulk_list_device writes it.
 * `sel` is copied by the call (the submit call included). GCK_E_INVALID_ARGUMENT, nothing launched,
 * for sel == NULL, mask == 0, mask & 1 (GCK_PERM_UNSPECIFIED cannot be selected), mask above 0xE,
 * reserved != 0, d_out_n == NULL, cap > 0 with all three output arrays NULL, a d_out_ids, d_out_pos
 * or d_out_n that is not 4-byte aligned, and everything the list device call refuses.
 * gck_device_compact_stats counts a filter request's chunks as a list device request's. */
#define GCK_SELECT_NO          (1u << GCK_PERM_NO)
#define GCK_SELECT_HAS         (1u << GCK_PERM_HAS)
#define GCK_SELECT_CONDITIONAL (1u << GCK_PERM_CONDITIONAL)
#define GCK_SELECT_LOOKUP      (GCK_SELECT_HAS | GCK_SELECT_CONDITIONAL)   /* LookupResources' rule */
typedef struct gck_select {
  uint32_t mask;        /* which Permissionships survive; bit GCK_PERM_UNSPECIFIED must be 0, mask != 0 */
  uint32_t reserved;    /* 0 */
  uint32_t* d_out_ids;  /* device, cap entries: the surviving check's varying id (ids[i] or first_id + i); may be NULL */
  uint32_t* d_out_pos;  /* device, cap entries: its position i in the request; may be NULL */
  uint8_t*  d_out_perm; /* device, cap entries: its GCK_PERM_*; may be NULL */
  size_t    cap;
  uint32_t* d_out_n;    /* device, required: the number of survivors of the whole request */
} gck_select;
int gck_filter_list_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                           uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                           const char* const* contexts, const size_t* context_lens, size_t n_contexts, int64_t now_us,
                           const gck_select* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                           uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision);
int gck_filter_submit_list_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                                  uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                                  const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                  int64_t now_us, const gck_select* sel, uint64_t* d_out_packed,
                                  gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, uint32_t flags,
                                  void* stream, gck_batch** out);

/* ---- cross filter requests (ABI 13, additive) ----------------------------------------
 * gck_check_bulk_cross_device / gck_check_submit_cross_device with the last step done on the device
 * too: "for each of these subjects, which of these resources" — the survivors of every row of the
 * finished plane, compacted by kernels into a CSR in the caller's device memory. Nothing but the two
 * count words (*d_out_n, *d_out_n_errs) ever needs to cross PCIe.
 * The check itself is the cross device call's, unchanged in every respect: the tiling and the block
 * layout read in place, the expansion on the device (check contexts, R >= GCK_CROSS_IDS, thin requests
 * and the other fallbacks), stream ordering and `flags`, consistency and the evaluated revision, the
 * error records (index = s * R + r) and the request errors. d_out_packed is required and is written
 * exactly as gck_check_bulk_cross_device writes it (a form without a plane is out of scope).
 * Check (s, r) survives iff it has no per-item error and (sel->mask >> perm) & 1. Row s has surv_s
 * survivors and keeps kept_s = row_limit ? min(surv_s, row_limit) : surv_s of them, the first in
 * ascending r (the first K permitted candidates of a ranked page).
 *   d_out_row_off: row_off[0] = 0, row_off[s + 1] = row_off[s] + kept_s; all S + 1 entries are always
 *     written, whatever cap is. With S == 0 only row_off[0] and *d_out_n (= 0) are written, besides the
 *     error count word; with R == 0 all S + 1 entries are 0 (and d_out_row_n, when given, S zeros).
 *   records: kept survivor j of row s has rank row_off[s] + j; its resource id (d_resources[r]), its
 *     position r in the resource list and its GCK_PERM_* go to every array that is not NULL iff
 *     rank < cap. Entries at and beyond min(total, cap) stay untouched.
 *   d_out_row_n[s] = surv_s (before row_limit) when the array is given; *d_out_n = row_off[S], always
 *     written.
 * Ids are reported as often as the resource list repeats them; the selection reads d_resources, which
 * stays valid until the synchronous call or the wait returns (the cross device call's lifetime rule).
 * A per-item error does not fail the call, as for the list filter: the errored check never survives
 * and the caller holds the count word.
 * `sel` is copied by the call (the submit call included). GCK_E_INVALID_ARGUMENT, nothing launched and
 * nothing written, for sel == NULL, a bad mask (gck_select's rule: 0, bit 0 set, above 0xE),
 * d_out_row_off == NULL, d_out_n == NULL, d_out_packed == NULL, cap > 0 with all three record arrays
 * NULL, a d_out_row_off, d_out_row_n, d_out_ids, d_out_col or d_out_n that is not 4-byte aligned, and
 * everything the cross device call refuses. gck_device_compact_stats counts the request as a cross
 * device request.
 * The mirror — per-resource rows of surviving subjects — is gck_filter_cross_cols_device, below.
 * Out of scope: a form without a plane; the three kernels of a one-tile plane fused into one launch. */
typedef struct gck_select_rows {
  uint32_t mask;           /* GCK_SELECT_*: as gck_select.mask (bit 0 clear, != 0, <= 0xE) */
  uint32_t row_limit;      /* 0: keep every survivor; else keep at most this many per subject, the first in list order */
  uint32_t* d_out_row_off; /* device, S + 1 entries, required */
  uint32_t* d_out_row_n;   /* device, S entries, may be NULL: survivors of row s BEFORE row_limit */
  uint32_t* d_out_ids;     /* device, cap entries, may be NULL: resources[r] of a kept survivor */
  uint32_t* d_out_col;     /* device, cap entries, may be NULL: its position r in the resource list */
  uint8_t*  d_out_perm;    /* device, cap entries, may be NULL: its GCK_PERM_* */
  size_t    cap;
  uint32_t* d_out_n;       /* device, required: kept survivors of the whole request (== row_off[S]) */
} gck_select_rows;         /* 64 bytes */
int gck_filter_cross_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                            const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                            size_t n_resources, const char* const* contexts, const size_t* context_lens,
                            size_t n_contexts, int64_t now_us, const gck_select_rows* sel, uint64_t* d_out_packed,
                            gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, void* stream,
                            uint64_t* out_revision);
int gck_filter_submit_cross_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                                   const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                   size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                   size_t n_contexts, int64_t now_us, const gck_select_rows* sel,
                                   uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                   uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out);

/* ---- cross filter requests by resource (ABI 13, additive) -----------------------------
 * The mirror of gck_filter_cross_device: "for each of these resources, which of these subjects" — an
 * access review, a share dialog, a notification fan-out — the survivors of every COLUMN of the same
 * finished plane, compacted by kernels into a CSR by resource in the caller's device memory. Nothing
 * but the two count words (*d_out_n, *d_out_n_errs) ever needs to cross PCIe.
 * The check itself is the cross device call's, unchanged in every respect, exactly as for
 * gck_filter_cross_device: the tiling and the block layout read in place, the expansion on the device
 * (check contexts, R >= GCK_CROSS_IDS, thin requests and the other fallbacks), stream ordering and
 * `flags`, consistency and the evaluated revision, the error records (index = s * R + r), the request
 * errors and the one-tile rule of the submit form. d_out_packed is required and is written exactly as
 * gck_check_bulk_cross_device writes it: the plane stays row-padded, S rows of ceil(R / 32) words.
 * Check (s, r) survives iff it has no per-item error and (sel->mask >> perm) & 1. Column r has surv_r
 * survivors and keeps kept_r = col_limit ? min(surv_r, col_limit) : surv_r of them, the first in
 * ascending s (the first K permitted subjects of the subject list's order).
 *   d_out_col_off: col_off[0] = 0, col_off[r + 1] = col_off[r] + kept_r; all R + 1 entries are always
 *     written, whatever cap is. With R == 0 only col_off[0] and *d_out_n (= 0) are written, besides the
 *     error count word; with S == 0 all R + 1 entries are 0 (and d_out_col_n, when given, R zeros).
 *   records: kept survivor j of column r has rank col_off[r] + j; its subject id (d_subjects[s]), its
 *     position s in the subject list and its GCK_PERM_* go to every array that is not NULL iff
 *     rank < cap. Entries at and beyond min(total, cap) stay untouched.
 *   d_out_col_n[r] = surv_r (before col_limit) when the array is given; *d_out_n = col_off[R], always
 *     written.
 * Ids are reported as often as the subject list repeats them; the selection reads d_subjects, which
 * stays valid until the synchronous call or the wait returns (the cross device call's lifetime rule).
 * A per-item error does not fail the call: the errored check never survives and the caller holds the
 * count word. An empty request (S == 0 or R == 0) does not touch gck_device_compact_stats; any other
 * is counted there as a cross device request.
 * `sel` is copied by the call (the submit call included). GCK_E_INVALID_ARGUMENT, nothing launched and
 * nothing written, for sel == NULL, a bad mask (gck_select's rule: 0, bit 0 set, above 0xE),
 * d_out_col_off == NULL, d_out_n == NULL, d_out_packed == NULL, cap > 0 with all three record arrays
 * NULL, a d_out_col_off, d_out_col_n, d_out_ids, d_out_row or d_out_n that is not 4-byte aligned, and
 * everything the cross device call refuses.
 * Cost: the selection kernels run one block per 64 resources, and each block walks all S rows of its
 * columns, 16 chunks of rows side by side. An in-place tile has S * ceil(R / 32) <= max_batch / 32 words, so that walk is
 * short; a huge, thin expanded plane (millions of subjects by a handful of resources) selects slowly
 * but correctly.
 * Out of scope: a form without a plane; the three kernels of a one-tile plane fused into one launch. */
typedef struct gck_select_cols {
  uint32_t mask;           /* GCK_SELECT_*: as gck_select.mask (bit 0 clear, != 0, <= 0xE) */
  uint32_t col_limit;      /* 0: keep every survivor; else keep at most this many per resource, the first in subject-list order */
  uint32_t* d_out_col_off; /* device, R + 1 entries, required */
  uint32_t* d_out_col_n;   /* device, R entries, may be NULL: survivors of column r BEFORE col_limit */
  uint32_t* d_out_ids;     /* device, cap entries, may be NULL: d_subjects[s] of a kept survivor */
  uint32_t* d_out_row;     /* device, cap entries, may be NULL: its position s in the subject list */
  uint8_t*  d_out_perm;    /* device, cap entries, may be NULL: its GCK_PERM_* */
  size_t    cap;
  uint32_t* d_out_n;       /* device, required: kept survivors of the whole request (== col_off[R]) */
} gck_select_cols;         /* 64 bytes */
int gck_filter_cross_cols_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                                 const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                 size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                 size_t n_contexts, int64_t now_us, const gck_select_cols* sel,
                                 uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                 uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision);
int gck_filter_submit_cross_cols_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                                        const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                        size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                        size_t n_contexts, int64_t now_us, const gck_select_cols* sel,
                                        uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                        uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out);

/* ---- group filter requests (ABI 13, additive) -------------------------------------------------
 * A candidate list per owner: S owners (d_owners) and a CSR of candidates — d_group_off, S + 1
 * offsets, and d_candidates, n ids — all in device memory: what a retrieval or ranking step returns,
 * its own top-K for each query or user. Check k (k < n) belongs to group s where off[s] <= k <
 * off[s + 1], and is (hdr, d_candidates[k], d_owners[s]) with vary == GCK_VARY_RESOURCE — owners are
 * subject ids, candidates resource ids — or (hdr, d_owners[s], d_candidates[k]) with GCK_VARY_SUBJECT:
 * for each of these documents, which of its own candidate users. 4 B per check and 4 B per group in.
 * d_out_packed (required) is the dense plane of ceil(n / 32) words, written exactly as
 * gck_check_bulk_uniform_device writes it for the same pairs (every word written, padding bits and
 * errored checks 0); the error records are (index = k, GCK_ITEM_*) ascending, under the device compact
 * calls' err_cap / *d_out_n_errs protocol. A per-item error does not fail the call: the check never
 * survives.
 * The selection, over the finished plane — gck_filter_cross_device's with "row s" read as "group s":
 *   surv_s = the checks of group s whose Permissionship `mask` selects, ascending in k;
 *   kept_s = group_limit ? min(surv_s, group_limit) : surv_s      (the first kept_s of them)
 *   d_out_row_off[0] = 0, d_out_row_off[s + 1] = d_out_row_off[s] + kept_s: all S + 1 entries written;
 *     an empty group has equal consecutive offsets.
 *   record j of group s has rank d_out_row_off[s] + j, j ascending with k; each given record array is
 *     written at a rank while rank < cap. Entries at and beyond min(total, cap) stay untouched.
 *   d_out_row_n[s] = surv_s (before group_limit) when the array is given; *d_out_n = row_off[S], always
 *     written.
 * The offsets are device memory, so no host code validates them: a kernel checks the rule off[0] == 0,
 * off[s] <= off[s + 1], off[S] == n, and a violation is GCK_E_INVALID_ARGUMENT from the synchronous
 * call or from the wait, the message naming the smallest offending s. The outputs are then unspecified,
 * but nothing outside them was written and nothing outside the inputs read: every kernel of the request
 * clamps what it takes from the offsets (a group index into [0, S - 1], a group's range into [0, n], a
 * record's rank below cap). S == 0 requires n == 0 and writes only row_off[0] = 0, *d_out_n = 0 and the
 * error count word; n == 0 with S > 0 reads no offset and writes S + 1 zero offsets (and S zero counts).
 * Stream ordering, flags / GCK_SUBMIT_ENGINE_STREAM, consistency and the evaluated revision are the
 * list device call's; d_owners, d_group_off and d_candidates stay valid and unchanged until the
 * synchronous call or the wait returns; `sel` is copied by the call. The synchronous form chunks n by
 * max_batch & ~31 as the uniform device form does; the submit form takes n <= max_batch. Each chunk is
 * expanded to 8-B pairs in the workspace by a kernel and runs as a uniform device chunk, counted in
 * gck_device_compact_stats as one (in place or expanded); an empty request is not counted.
 * GCK_E_INVALID_ARGUMENT, nothing launched and nothing written, for sel == NULL, a bad mask
 * (gck_select's rule), a header whose `reserved` is not 0, a vary that is neither GCK_VARY_*,
 * d_out_row_off, d_out_n or d_out_packed NULL, cap > 0 with all three record arrays NULL, n or S at or
 * above 2^32, n > 0 with S == 0, a null input with n > 0, a d_out_packed that is not 8-byte aligned, any
 * other device pointer that is not 4-byte aligned, and a context slot beyond n_contexts.
 * Out of scope: the joins reading the CSR without the pair expansion; shaped (multi-header) groups; a
 * form without a plane; the kernels of a one-chunk request fused. */
typedef struct gck_select_groups {
  uint32_t mask;           /* GCK_SELECT_*: gck_select's rule (bit 0 clear, != 0, <= 0xE) */
  uint32_t group_limit;    /* 0: keep every survivor; else at most this many per group, the first in the group's order */
  uint32_t* d_out_row_off; /* device, S + 1 entries, required */
  uint32_t* d_out_row_n;   /* device, S entries, may be NULL: survivors of group s BEFORE group_limit */
  uint32_t* d_out_ids;     /* device, cap entries, may be NULL: d_candidates[k] of a kept survivor */
  uint32_t* d_out_pos;     /* device, cap entries, may be NULL: its position k in d_candidates (global, not in-group) */
  uint8_t*  d_out_perm;    /* device, cap entries, may be NULL: its GCK_PERM_* */
  size_t    cap;
  uint32_t* d_out_n;       /* device, required: kept survivors of the whole request (== row_off[S]) */
} gck_select_groups;       /* 64 bytes */
int gck_filter_groups_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t vary,
                             const uint32_t* d_owners, size_t n_owners, const uint32_t* d_group_off,
                             const uint32_t* d_candidates, size_t n_candidates, const char* const* contexts,
                             const size_t* context_lens, size_t n_contexts, int64_t now_us,
                             const gck_select_groups* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                             size_t err_cap, uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision);
int gck_filter_submit_groups_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t vary,
                                    const uint32_t* d_owners, size_t n_owners, const uint32_t* d_group_off,
                                    const uint32_t* d_candidates, size_t n_candidates, const char* const* contexts,
                                    const size_t* context_lens, size_t n_contexts, int64_t now_us,
                                    const gck_select_groups* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                                    size_t err_cap, uint32_t* d_out_n_errs, uint32_t flags, void* stream,
                                    gck_batch** out);

/* ---- recheck requests (ABI 13, additive) ----------------------------------------------
 * "What changed since the plane I kept?" A list or cross device request is evaluated at the current
 * revision and compared on the device with the caller's previous plane of the same request (device
 * memory, the layout the call itself writes). The answer is the new plane plus the ordered records of
 * the checks whose value changed; nothing but the count words (*d_out_n, *d_out_n_errs) needs to cross
 * PCIe. The use: an ACL column of a search or vector index, a per-user cache of visible documents, a
 * denormalised permission-set table — anything that keeps an answer across Watch batches
 * (gck_apply_updates) and must patch it.
 * A transition is a pair (old value v, new value w) of GCK_PERM_*, v != w. `transitions` has bit
 * 4 * v + w set when that pair is selected; it is valid iff it is non-zero and lies within
 * GCK_CHANGE_ANY. Value 0 (GCK_PERM_UNSPECIFIED: an errored check, or a previous plane that is NULL) is
 * a legal end of a transition: a check that had a GCK_ITEM_* error and now is HAS is a real change. A
 * change's transition byte is 4 * old + new, its bit index in `transitions`.
 * d_prev_packed: the previous plane, ceil(n / 32) words (list) or S rows of ceil(R / 32) words (cross),
 * 8-byte aligned; NULL reads as all zeros, so a first call with GCK_CHANGE_GAINED yields the initial
 * grant set. Its padding lanes may hold anything: a change's position is below n, its column below R.
 * Its range must not overlap d_out_packed's. d_out_packed is required, is written exactly as
 * gck_check_bulk_list_device / gck_check_bulk_cross_device write it, and is the previous plane of the
 * caller's next call.
 * The check itself is the list or cross device call's, unchanged in every respect (tiling, in-place
 * and expanded paths, fallbacks, stream ordering and `flags`, consistency, error records, the
 * evaluated revision). The comparison is a request-level step behind the last chunk or tile of the
 * synchronous form, and in the wait of a submitted batch.
 *   gck_select_changes (list form): records (varying id, position, transition byte) in ascending
 *     position; record k goes to every array that is not NULL iff k < cap; *d_out_n = the number of
 *     changes of the whole request, always written (for n == 0 too).
 *   gck_select_row_changes (cross form): a CSR by subject. d_out_row_off[0] = 0, row_off[s + 1] =
 *     row_off[s] + the changes of row s; all S + 1 entries always written (S == 0: row_off[0] alone;
 *     R == 0: S + 1 zeros). Change j of row s, ascending in r, has rank row_off[s] + j; its resource id
 *     (d_resources[r]), its column r and its transition byte go to every array that is not NULL iff
 *     rank < cap. *d_out_n = row_off[S], always written. There is no per-row limit.
 * Entries at and beyond min(total, cap) stay untouched. The structs are copied by the call (the submit
 * call included). GCK_E_INVALID_ARGUMENT, nothing launched and nothing written, for a NULL struct, bad
 * `transitions`, reserved != 0, a missing required pointer (d_out_n; d_out_row_off; d_out_packed of a
 * request call; the new plane of a plane-only call with checks), cap > 0 with all three record arrays
 * NULL, a plane that is not 8-byte aligned or any other pointer that is not 4-byte aligned, a
 * d_prev_packed range that overlaps d_out_packed's, and everything the underlying call refuses.
 * gck_device_compact_stats counts a recheck as the list or cross device request it is.
 * Out of scope: a group-segmented form (a group request's plane is dense: use the dense form and map
 * positions with the offsets), and a diff combined with a survivor filter in one call. */
#define GCK_CHANGE_GAINED 0x00CCu /* {UNSPECIFIED, NO} -> {HAS, CONDITIONAL} */
#define GCK_CHANGE_LOST   0x3300u /* {HAS, CONDITIONAL} -> {UNSPECIFIED, NO} */
#define GCK_CHANGE_ANY    0x7BDEu /* every pair of different values */
typedef struct gck_select_changes {
  uint32_t transitions;  /* GCK_CHANGE_*: != 0, within GCK_CHANGE_ANY */
  uint32_t reserved;     /* 0 */
  uint32_t* d_out_ids;   /* device, cap entries, may be NULL: the changed check's varying id (ids[i] or first_id + i) */
  uint32_t* d_out_pos;   /* device, cap entries, may be NULL: its position i in the request */
  uint8_t*  d_out_trans; /* device, cap entries, may be NULL: 4 * old + new */
  size_t    cap;
  uint32_t* d_out_n;     /* device, required: the changes of the whole request */
} gck_select_changes;    /* 48 bytes */
typedef struct gck_select_row_changes {
  uint32_t transitions;    /* GCK_CHANGE_*: != 0, within GCK_CHANGE_ANY */
  uint32_t reserved;       /* 0 */
  uint32_t* d_out_row_off; /* device, S + 1 entries, required */
  uint32_t* d_out_ids;     /* device, cap entries, may be NULL: resources[r] of a change */
  uint32_t* d_out_col;     /* device, cap entries, may be NULL: its position r in the resource list */
  uint8_t*  d_out_trans;   /* device, cap entries, may be NULL: 4 * old + new */
  size_t    cap;
  uint32_t* d_out_n;       /* device, required: the changes of the whole request (== row_off[S]) */
} gck_select_row_changes;  /* 56 bytes */
/* The comparison alone, for a caller that already holds both planes (any dense plane: a uniform,
 * shaped, list or group request's; or a cross plane). d_ids: the n varying ids, or NULL for
 * first_id + i. Synchronous on `stream`; needs a committed snapshot, as every device call does. */
int gck_diff_planes_device(gck_engine* e, const uint64_t* d_old, const uint64_t* d_new, size_t n, const uint32_t* d_ids,
                           uint32_t first_id, const gck_select_changes* sel, void* stream);
int gck_diff_cross_planes_device(gck_engine* e, const uint64_t* d_old, const uint64_t* d_new, size_t n_subjects,
                                 size_t n_resources, const uint32_t* d_resources, const gck_select_row_changes* sel,
                                 void* stream);
int gck_recheck_list_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                            uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                            const char* const* contexts, const size_t* context_lens, size_t n_contexts, int64_t now_us,
                            const uint64_t* d_prev_packed, const gck_select_changes* sel, uint64_t* d_out_packed,
                            gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, void* stream,
                            uint64_t* out_revision);
int gck_recheck_submit_list_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                                   uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                                   const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                   int64_t now_us, const uint64_t* d_prev_packed, const gck_select_changes* sel,
                                   uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                   uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out);
int gck_recheck_cross_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                             const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                             size_t n_resources, const char* const* contexts, const size_t* context_lens,
                             size_t n_contexts, int64_t now_us, const uint64_t* d_prev_packed,
                             const gck_select_row_changes* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                             size_t err_cap, uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision);
int gck_recheck_submit_cross_device(gck_engine* e, const gck_consistency* cs, const gck_uniform* hdr,
                                    const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                    size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                    size_t n_contexts, int64_t now_us, const uint64_t* d_prev_packed,
                                    const gck_select_row_changes* sel, uint64_t* d_out_packed,
                                    gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, uint32_t flags,
                                    void* stream, gck_batch** out);

/* ---- lookups (Client.LookupResources / LookupSubjects, client/client.go:508-599) -------- */
/* Ids of the `resource_type` objects on which the subject has `permission` — HAS or CONDITIONAL,
 * out_perm[k] says which — ascending. Every object of the type is checked on the device (the
 * check path's stages, candidates generated and answers compacted there). *out_n = the number of
 * ids; when it exceeds `cap` nothing is written and GCK_E_CAPACITY is returned: call again with
 * cap >= *out_n (the result of the last lookup is kept per thread, so the retry does not sweep
 * again). Errors: GCK_E_NOT_FOUND (unknown type / permission / subject relation),
 * GCK_E_INVALID_ARGUMENT (a candidate hit the depth budget), GCK_E_REVISION (consistency). */
int gck_lookup_resources(gck_engine* e, const gck_consistency* cs, uint16_t resource_type, uint16_t permission,
                         uint16_t subject_type, uint16_t subject_relation, uint32_t subject_id, int64_t now_us,
                         uint32_t* out_ids, uint8_t* out_perm, size_t cap, size_t* out_n);
/* Ids of the `subject_type` objects (with `subject_relation`, GCK_ELLIPSIS for plain objects)
 * that have `permission` on one resource, ascending; same protocol. As SpiceDB's LookupSubjects:
 * the candidates are the subjects on the relationships the permission's rewrite reaches from the
 * resource (a walk on the device), each checked on the check path; a wildcard grant is reported
 * once, as GCK_ID_WILDCARD (last), not as every subject of the type. */
int gck_lookup_subjects(gck_engine* e, const gck_consistency* cs, uint16_t resource_type, uint32_t resource_id,
                        uint16_t permission, uint16_t subject_type, uint16_t subject_relation, int64_t now_us,
                        uint32_t* out_ids, uint8_t* out_perm, size_t cap, size_t* out_n);

/* Lookups among the caller's candidates (ABI 13, additive): of the `n_candidates` ids of
 * `candidates`, those on which the subject has `permission` (HAS or CONDITIONAL, out_perm[k] says
 * which) — in the candidates' order, an id as often as the list repeats it. The candidates run as
 * one list request (above), 4 B per candidate in, 2 bits out, and the plane is scanned on the host.
 * candidates == NULL: every object of the type, as the one range [0, object count) — the result
 * of gck_lookup_resources. Protocol and errors are gck_lookup_resources': *out_n, GCK_E_CAPACITY
 * and the per-thread kept result (a retry with the same arguments and candidates at the same
 * explicit now_us does not check again); a candidate with a per-item error fails the call. */
int gck_lookup_resources_among(gck_engine* e, const gck_consistency* cs, uint16_t resource_type, uint16_t permission,
                               uint16_t subject_type, uint16_t subject_relation, uint32_t subject_id,
                               const uint32_t* candidates, size_t n_candidates, int64_t now_us, uint32_t* out_ids,
                               uint8_t* out_perm, size_t cap, size_t* out_n);
/* The mirror: of the candidate subjects (of `subject_type` with `subject_relation`), those that
 * have `permission` on one resource. A candidate list is required (NULL with n_candidates > 0 is
 * GCK_E_INVALID_ARGUMENT). No wildcard entry is reported: a wildcard grant makes every candidate
 * match. */
int gck_lookup_subjects_among(gck_engine* e, const gck_consistency* cs, uint16_t resource_type, uint32_t resource_id,
                              uint16_t permission, uint16_t subject_type, uint16_t subject_relation,
                              const uint32_t* candidates, size_t n_candidates, int64_t now_us, uint32_t* out_ids,
                              uint8_t* out_perm, size_t cap, size_t* out_n);

/* ---- partitioned graphs (graphs above one GPU's 288 GB) ----------------
 * Rank r of `world` (one process per GPU) owns the objects whose names hash to it
 * (gck_partition_owner_name, below: decided from the name, before anything is interned; the
 * owner gives the id, local * world + r, so gck_partition_owner(id) = id mod world names the same
 * rank). Every rank reads the whole export / Watch stream and keeps only (every ingest path
 * filters — gck_part_add_tuples_text_with, gck_add_tuples, gck_load_csr, gck_apply_updates —
 * none stores another rank's rows):
 *   - the relationships of the objects it owns;
 *   - the schema's hub hierarchy (the userset and wildcard relationships of "hub" relations —
 *     nested groups, teams — which usersets and arrows point at and which allow no caveat or
 *     expiration), replicated;
 *   - the direct hub memberships of the subjects it owns (their side of the label join: a hub
 *     membership goes to its subject's owner, not its object's).
 * All ranks then check one batch together — every rank calls with the same items and gets every
 * result: the label join (a subject's owner sends its slot to the resource's owner, which decides
 * the check), then an exact-depth level loop over what it left, with intersection, exclusion,
 * all() and caveats, exchanging frontier entries and join state per level. The exchange goes over
 * RCCL inside libgck (gck_part_init + gck_part_check) or over the caller's transport
 * (gck_part_check_with). Check-time caveat contexts are not taken in this mode. A partitioned
 * engine refuses gck_check_bulk*, lookups and snapshot files. */
/* Before the first snapshot: this engine is rank `rank` of `world` (1 = not partitioned). */
int gck_set_partition(gck_engine* e, uint32_t rank, uint32_t world);
uint32_t gck_partition_owner(uint32_t object_id, uint32_t world);

/* A caller's exchange between the ranks of a partition. Device buffers on the engine's device,
 * ordered on `stream` (the engine's work before the call is on it; the engine reads `recv` after
 * the call, on it): the transport may enqueue the transfer there (RCCL) or synchronise the stream
 * and complete it before returning (a host-staged transport).
 *   alltoallv: this rank sends send_bytes[d] bytes to rank d and receives recv_bytes[s] bytes
 *     from rank s; the blocks lie back to back in rank order in `send` and `recv` (the engine
 *     passes 0 for itself). Both sides know the sizes: the engine exchanges them first.
 *   allreduce_max_u8: in place, element-wise MAX over the ranks of n bytes.
 * Each returns 0, or non-zero on failure (the check then fails with GCK_E_DEVICE). */
typedef struct gck_transport {
  void* ctx;
  int (*alltoallv)(void* ctx, const void* d_send, const uint64_t* send_bytes, void* d_recv,
                   const uint64_t* recv_bytes, void* stream);
  int (*allreduce_max_u8)(void* ctx, void* d_buf, uint64_t n, void* stream);
} gck_transport;

/* Object names on a partitioned engine (world > 1; SURVEY.md §8e: owner = hash(type, id) mod G).
 * A name's owner is gck_partition_owner_name(type, name) — FNV-1a over the type (2 bytes, little
 * endian) and the name's bytes, finalised, mod world — decided before anything is interned, and
 * only the owner gives it an id: local * world + owner, in the order the owner meets its names, so
 * that gck_partition_owner(id) is the same rank and every rank holds the same id for a name. A rank
 * keeps only the names of what it owns and of what its rows and checks reference (the replicated
 * hub hierarchy among them); local interning of a new name (gck_intern with GCK_INTERN_CREATE,
 * gck_add_tuples_text, gck_apply_updates_text) is refused with GCK_E_STATE on such an engine.
 * Both calls below are collective: every rank of the partition calls them, in the same order. */
uint32_t gck_partition_owner_name(uint16_t type, const char* name, size_t len, uint32_t world);
/* Every rank its own names (types[i], names[i] of lens[i] bytes) -> out_ids[i]: "*" is
 * GCK_ID_WILDCARD; a name the owner does not know is created with GCK_INTERN_CREATE, else
 * GCK_ID_ABSENT (check items: build them with this, so that every rank has the same items). With
 * GCK_INTERN_CREATE every rank's object counts become world x the largest owner's count. */
int gck_part_intern_with(gck_engine* e, const gck_transport* t, const uint16_t* types, const char* const* names,
                         const uint32_t* lens, size_t n, uint32_t flags, uint32_t* out_ids);
/* The export stream's relationships as text (gck_add_tuples_text's format), the same text on every
 * rank, between gck_begin_snapshot and gck_commit_snapshot: each rank keeps what it owns (decided
 * from the names) and interns the names of those relationships only, through their owners. */
int gck_part_add_tuples_text_with(gck_engine* e, const gck_transport* t, const char* text, size_t len);
/* The names this engine's interner holds for a type (on a partitioned engine: its own objects'
 * and those its rows and checks referenced; otherwise every named object). */
int gck_interned_names(gck_engine* e, uint16_t type, uint32_t* out);

/* The partitioned check over the caller's transport: n device items (the same on every rank) in,
 * every result out on every rank (d_out_perm / d_out_err, device). `now_us` 0 = rank 0's clock. */
int gck_part_check_with(gck_engine* e, const gck_transport* t, const gck_item* d_items, size_t n, int64_t now_us,
                        uint8_t* d_out_perm, int32_t* d_out_err, void* stream);

/* The same over RCCL inside libgck (xGMI between the GPUs of a node: grouped ncclSend / ncclRecv,
 * ncclAllReduce). Rank 0 makes the id (gck_part_unique_id), the caller hands the same bytes to
 * every rank (any transport: a TCP store, MPI, a file), and each rank joins with gck_part_init
 * after gck_set_partition. */
#define GCK_PART_UNIQUE_ID_BYTES 128
int gck_part_unique_id(uint8_t out[GCK_PART_UNIQUE_ID_BYTES]);
int gck_part_init(gck_engine* e, const uint8_t id[GCK_PART_UNIQUE_ID_BYTES]);
int gck_part_check(gck_engine* e, const gck_item* d_items, size_t n, int64_t now_us, uint8_t* d_out_perm,
                   int32_t* d_out_err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCK_H */
