/*
 * iris_hip.h — C ABI of the MI355X-native masked-Hamming iris-matching engine.
 *
 * This is the drop-in boundary for the hot path of recmo/mpc-iris-code
 * (reference v0.8.0).  Every entry point names the reference interface it
 * replaces (path:line inside the reference repository).  The Rust-side
 * binding a maintainer would add (`src/arch/hip.rs`) is in INTEGRATION.md.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Host buffers are owned by the caller;
 *    device buffers are owned by the library behind opaque handles.
 *  - Every function returns an int status: 0 = ok, < 0 = error.  The message
 *    of the last error on the calling thread is returned by iris_last_error().
 *    (The reference panics on `assert_eq!(out.len(), db.len())`,
 *    src/lib.rs:43,70; the Rust shim maps IRIS_E_ARG back to that panic.)
 *  - All calls are blocking: when they return, host outputs are filled, as the
 *    reference's synchronous `batch_process` (src/lib.rs:42,69).
 *  - Handles are thread-safe: calls on one device are serialised internally
 *    (the reference engines are `Sync` and shared by rayon workers).
 *  - Calls switch to their handle's device internally and leave the calling
 *    thread's current HIP device as they found it.
 *  - Record layouts are the reference's in-memory / on-disk layouts
 *    (bytemuck views, little-endian):
 *      Bits        = uint64_t[200]            (src/bits.rs:13-15)      1600 B
 *      EncodedBits = uint16_t[12800]          (src/encoded_bits.rs:13-15) 25600 B
 *      Template    = { Bits pattern; Bits mask; } (src/template.rs:11-29) 3200 B
 *    On the device the library keeps its own lane-interleaved layout
 *    (DESIGN.md §3); conversion happens on upload / read-back.
 */
#ifndef IRIS_HIP_H
#define IRIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Geometry: src/lib.rs:10-12, src/bits.rs:10-11 */
#define IRIS_COLS 200
#define IRIS_ROWS 64
#define IRIS_BITS 12800
#define IRIS_LIMBS 200
#define IRIS_ROTATIONS 31   /* r = k - 15, k = 0..30 (src/lib.rs:34,61) */
#define IRIS_MAX_ROTATION 15

/* Status codes */
#define IRIS_OK 0
#define IRIS_E_ARG (-1)       /* bad argument / length mismatch            */
#define IRIS_E_HIP (-2)       /* HIP runtime error                          */
#define IRIS_E_NOMEM (-3)     /* device or host allocation failed          */
#define IRIS_E_NODEV (-4)     /* no usable gfx950 device                    */
#define IRIS_E_RANGE (-5)     /* index range outside the database          */
#define IRIS_E_IO (-6)        /* file open / read / write failed            */
#define IRIS_E_FORMAT (-7)    /* malformed JSON template file               */

/* Database record kinds */
#define IRIS_KIND_MASKS 1     /* records are Bits (the resolver's masks file, src/main.rs:455-469) */
#define IRIS_KIND_SHARES 2    /* records are EncodedBits (a participant's share file, src/main.rs:386-400) */
#define IRIS_KIND_TEMPLATES 3 /* records are Template (plaintext masked Hamming, src/template.rs) */

/* Device layouts of a database (iris_db_create_ex) */
#define IRIS_LAYOUT_DEFAULT 0 /* TILES                                          */
#define IRIS_LAYOUT_LANES 1   /* record-per-lane blocks of 64 (VALU kernels)   */
#define IRIS_LAYOUT_TILES 2   /* 32-record MFMA tiles (fp4 / i8 kernels)        */
/* (3 was the search-only TRITS template layout of rounds 2-3; removed, refused as unknown) */

typedef struct iris_template {
    uint64_t pattern[IRIS_LIMBS];
    uint64_t mask[IRIS_LIMBS];
} iris_template_t;

/* Result of a search: the reference resolver's (min_distance, min_index)
 * pair (src/main.rs:581-582, 616-621) plus the exact fraction behind it.   */
typedef struct iris_match {
    double distance;   /* f64 value, +inf when no template has a valid rotation */
    uint64_t index;    /* global template index; UINT64_MAX when distance is +inf */
    uint32_t num;      /* uneq count of the winning rotation                   */
    uint32_t den;      /* jointly-valid bit count of the winning rotation      */
    int32_t rotation;  /* winning r in -15..15 (lowest r on ties); 0 if none   */
    uint32_t reserved;
} iris_match_t;

typedef struct iris_device iris_device_t;
typedef struct iris_db iris_db_t;
typedef struct iris_engine iris_engine_t;
typedef struct iris_pending iris_pending_t;
/* The handles of iris_template_matches_async, iris_template_topk_async and
 * iris_template_report_async: the same opaque struct under names of their own.  Each of the four
 * waits refuses (IRIS_E_ARG) and leaves alone a handle another submission made. */
typedef iris_pending_t iris_pending_matches_t;
typedef iris_pending_t iris_pending_topk_t;
typedef iris_pending_t iris_pending_report_t;

/* ---------------------------------------------------------------- errors */
const char *iris_last_error(void);
const char *iris_version(void);
/* Runtime configuration, read from the environment once when a device opens:
 * "key=value ..." into buf (NUL-terminated, truncated to len); *needed (may be
 * NULL) receives the full length without the NUL.  dev == NULL: what a device
 * opened now would use.  Production knobs: IRIS_READAHEAD, IRIS_AUTO_RESIDENT,
 * IRIS_GROUP_TIMEOUT_MS, IRIS_COPY_HELPERS (process-wide).  Test-only hooks
 * (IRIS_TILES_PER_WAVE, IRIS_FUSED_REDUCE, IRIS_BATCH_KERNEL, IRIS_SCHEDULE,
 * IRIS_LOAD_PREAD, IRIS_LOAD_WINDOWS, IRIS_GROUP_DELAY_US, IRIS_GROUP_STALL,
 * IRIS_GROUP_UNORDERED, IRIS_UPLOAD, IRIS_READAHEAD_WINDOW, IRIS_RESIDENT_BUDGET_MB,
 * IRIS_READAHEAD_PACKED, IRIS_READAHEAD_WINDOW_MAX) take effect only with IRIS_TEST_HOOKS=1;
 * otherwise they are ignored and listed as "ignored=...".  With dev != NULL the
 * device's own facts follow: numa_node= (host NUMA node of its PCI function, -1
 * unknown), upload_gbps=P/R (recent rates of large writes through the pinned
 * slots / the runtime's copy, GB/s; 0 = not measured yet), resident= (the
 * record files it keeps resident for host-slice calls: count and bytes) and
 * readahead_windows=L/R/M (read-ahead launches of host-output engine calls since
 * the last iris_device_reset_stats, the records they computed, the largest
 * window in records) and abandoned_inits=P/T (RCCL communicator inits of this
 * device that a group formation gave up on at its bound: still pending inside
 * RCCL / all in this process; while one is pending the device forms no further
 * multi-rank group in this process).  group_init_timeout_ms= is the bound of
 * forming a group (IRIS_GROUP_TIMEOUT_MS, else 120000). */
int iris_config(const iris_device_t *dev, char *buf, size_t len, size_t *needed);

/* --------------------------------------------------------------- devices */
int iris_device_count(int *count);
/* Opens a HIP device (must be gfx950).  Owns one non-blocking HIP stream. */
int iris_device_open(int ordinal, iris_device_t **out);
int iris_device_close(iris_device_t *dev);
int iris_device_synchronize(iris_device_t *dev);
/* The device's stream as a hipStream_t, for callers that order their own work. */
int iris_device_stream(iris_device_t *dev, void **stream);
/* Free and total device memory in bytes (sizing a resident database: a template
 * takes 3200 B, a mask 1600 B, a share 25600 B; the reference mmaps its files
 * instead, src/main.rs:389,458). */
int iris_device_memory(iris_device_t *dev, size_t *free_bytes, size_t *total_bytes);
/* Kernel timing with HIP events recorded on the device stream around every
 * launch of the named kernel family ("template_search", "template_counts",
 * "masks", "shares", "shares_batch" (items = records x queries), "masks_batch" and
 * "masks_batch_resolve" (the same), ...).  Disabled by default.  Beside the
 * timed "shares_batch" entry of a call on a TILES database, "shares_batch_large",
 * "shares_batch_split" and "shares_batch_single" count the passes it ran in each
 * kernel form (launches = passes, items = their rows, no time of their own). */
int iris_device_set_profiling(iris_device_t *dev, int enabled);
int iris_device_kernel_stats(iris_device_t *dev, const char *kernel, uint64_t *launches,
                             double *total_ms, uint64_t *items);
/* The largest launch of the named kernel family since the last reset: its items
 * (records) and its duration (ms; the latest of equal-sized ones); 0 / 0 if none.
 * A walk's biggest read-ahead window, for its HBM fraction. */
int iris_device_kernel_stats_largest(iris_device_t *dev, const char *kernel, uint64_t *items, double *ms);
int iris_device_reset_stats(iris_device_t *dev);
/* Raw device memory for outputs that stay on the GPU (e.g. per-template distances). */
int iris_device_alloc(iris_device_t *dev, size_t bytes, void **ptr);
int iris_device_free(iris_device_t *dev, void *ptr);
int iris_memcpy_d2h(iris_device_t *dev, void *host, const void *device, size_t bytes);
int iris_memcpy_h2d(iris_device_t *dev, void *device, const void *host, size_t bytes);

/* -------------------------------------------------------------- databases
 * Device-resident database of `kind` records.  Replaces the mmap'd share /
 * masks files the reference keeps in host memory (src/main.rs:389,458).     */
int iris_db_create(iris_device_t *dev, int kind, uint64_t capacity, iris_db_t **out);
/* As iris_db_create with an explicit device layout (IRIS_LAYOUT_*).  The
 * layout only selects the kernel family; results are identical. */
int iris_db_create_ex(iris_device_t *dev, int kind, uint64_t capacity, int layout, iris_db_t **out);
int iris_db_layout(const iris_db_t *db, int *layout);
int iris_db_destroy(iris_db_t *db);
int iris_db_len(const iris_db_t *db, uint64_t *len);
int iris_db_capacity(const iris_db_t *db, uint64_t *cap);
int iris_db_kind(const iris_db_t *db, int *kind);
/* Appends n host records (reference layout) at the end. */
int iris_db_append(iris_db_t *db, const void *records, uint64_t n);
/* Overwrites records [index, index+n) (must lie inside [0, len]) — grows len if needed. */
int iris_db_write(iris_db_t *db, uint64_t index, const void *records, uint64_t n);
/* Reads records [first, first+n) back to the reference layout. */
int iris_db_read(const iris_db_t *db, uint64_t first, uint64_t n, void *records);
/* Appends n synthetic records generated on the device by the counter-based
 * generator of DESIGN.md §5 (template index t = global_index0 + i): uniform
 * random bits / u16 as the reference's `rng.gen()` (src/bits.rs:95-101,
 * src/encoded_bits.rs:81-87, src/template.rs:67-74). */
int iris_db_generate(iris_db_t *db, uint64_t n, uint64_t seed, uint64_t global_index0);
int iris_db_clear(iris_db_t *db);
/* Drops the records [len, current length) (no device work; later appends overwrite them). */
int iris_db_truncate(iris_db_t *db, uint64_t len);

/* ---------------------------------------------------------------- host residency
 * The reference's participant and resolver mmap their record file once and
 * call batch_process(out, chunk) on 20 000-record slices of the mapping
 * (src/main.rs:389-391, 426-431; 458-460, 511-516).  iris_db_attach_host
 * declares that db's records [0, n) are the n records of the host array at
 * `host` (e.g. that mapping): with upload != 0 the (empty) database receives
 * them now; with upload == 0 it must already hold exactly them (e.g. loaded
 * from the same file with iris_db_load_file; the first, middle and last
 * record are compared).  From then on iris_engine_batch_process_host on any
 * record range inside the array (same kind, whole records) runs the engine on
 * the resident copy and uploads nothing; other slices still upload.  The host
 * array must stay unchanged while attached; any write to the database
 * (append, write, generate, clear, truncate, load, prepare) or its
 * destruction detaches it. */
int iris_db_attach_host(iris_db_t *db, const void *host, uint64_t n, int upload);
int iris_db_detach_host(iris_db_t *db);

/* ---------------------------------------------------------------- on-disk formats
 * Record files hold the raw little-endian bytes of a record slice
 * (bytemuck::bytes_of): `prepare` writes them and `participant` / `resolver`
 * mmap them (src/main.rs:299-309,341,353-357,386-400,455-469):
 *   IRIS_KIND_MASKS      *.masks    Bits        1600 B
 *   IRIS_KIND_SHARES     *.share-i  EncodedBits 25600 B
 *   IRIS_KIND_TEMPLATES  raw Template (pattern then mask) 3200 B
 * iris_db_load_file appends records [first, first+count) of the file
 * (count = UINT64_MAX: to the end): the mapped file's page-cache pages are
 * registered with the device and copied by DMA in ~64-MB chunks, overlapping
 * the layout transpose (if registration fails, the range is read through two
 * pinned buffers by reader threads instead; IRIS_LOAD_PREAD=1 forces it); *loaded
 * (may be NULL) receives the number appended.  A file whose size is not a
 * multiple of the record size is rejected (IRIS_E_ARG), as the reference's
 * try_cast_slice does ("Share file … invalid.", src/main.rs:390-393,459-462). */
int iris_db_load_file(iris_db_t *db, const char *path, uint64_t first, uint64_t count, uint64_t *loaded);
/* Writes records [first, first+n) of db to `path` (created / truncated) in
 * the same raw format. */
int iris_db_save_file(const iris_db_t *db, const char *path, uint64_t first, uint64_t n);
/* JSON template files: a top-level array of {"pattern": hex, "mask": hex}
 * objects, each Bits the hex of its 1600 LE bytes (serde form of Template,
 * src/template.rs:11-29, src/bits.rs:74-93; read like the streaming
 * iter_json_array, src/json_stream.rs:53-60).  Read: up to cap templates go
 * to out (out may be NULL to count); *n is the number in the file;
 * IRIS_E_RANGE if it exceeds cap, IRIS_E_FORMAT with the byte offset on
 * malformed input.  Write: compact JSON, lowercase hex (hex::serialize). */
int iris_templates_read_json(const char *path, iris_template_t *out, uint64_t cap, uint64_t *n);
int iris_templates_write_json(const char *path, const iris_template_t *templates, uint64_t n);

/* ---------------------------------------------------------------- share preparation
 * The reference's `prepare` (src/main.rs:333-361) on the device: for the
 * templates [first, first+n) of a template database, appends n records to
 * each of the `parties` share databases — EncodedBits::share(parties) of
 * encode(template) (src/encoded_bits.rs:23-38, src/lib.rs:16-26): parties-1
 * uniformly random shares and a last one = encode - sum(rest) mod 2^16 —
 * and, if masks is not NULL, the template's mask to the masks database.
 * Randomness: ChaCha with `rounds` = 8, 12 or 20 (Bernstein's 64-bit-nonce
 * form) in counter mode under the caller's 256-bit key and 64-bit nonce (key
 * from a CSPRNG such as getrandom).  The reference uses rand 0.8.5's
 * thread_rng, a reseeded ChaCha12 (rand_chacha 0.3.1): 12 is its round count
 * and the recommended value.  Share j < parties-1 of global template index
 * g = index_base + first + i, elements 32b..32b+31 = the 32 LE u16 of
 * keystream block (g*(parties-1) + j)*400 + b.  Deterministic given
 * (key, nonce, g), so shards prepared on different GPUs never reuse a block. */
int iris_prepare_shares(const iris_db_t *templates, uint64_t first, uint64_t n, uint64_t index_base,
                        const uint8_t key[32], uint64_t nonce, uint32_t rounds, uint32_t parties,
                        iris_db_t *const *shares, iris_db_t *masks);

/* ---------------------------------------------------------------- engines
 * MasksEngine::new(&Bits)            src/lib.rs:60-67
 * DistanceEngine::new(&EncodedBits)  src/lib.rs:33-40
 * Template engine (query Template vs Template DB; src/template.rs:43-64)
 * Each builds the 31 rotated query copies once, as the reference does.     */
int iris_masks_engine_new(iris_device_t *dev, const uint64_t query_mask[IRIS_LIMBS], iris_engine_t **out);
int iris_distance_engine_new(iris_device_t *dev, const uint16_t query[IRIS_BITS], iris_engine_t **out);
int iris_template_engine_new(iris_device_t *dev, const iris_template_t *query, iris_engine_t **out);
int iris_engine_destroy(iris_engine_t *engine);

/* batch_process(&self, out: &mut [[u16; 31]], db: &[T])   src/lib.rs:42-52, 69-79
 * Masks engine: out[i][k] = dot_bool(rot(query_mask, k-15), db[i])
 * Distance engine: out[i][k] = dot_u16(rot(query, k-15), db[i])  (mod 2^16)
 * Device-resident form: processes db records [first, first+n); out is a host
 * array of n*31 uint16_t.  The engine kind must match the DB kind. */
int iris_engine_batch_process(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                              uint16_t *out);
/* As iris_engine_batch_process, with out_device a DEVICE array of n*31
 * uint16_t (for pipelines that keep the results on the GPU).  Blocking: when
 * it returns the rows are in device memory, visible to any reader (another
 * stream, a copy engine, another process's mapping) -- a participant-sized
 * range returns on a completion word its kernel writes after storing the rows
 * through L2, before the launch itself has retired. */
int iris_engine_batch_process_device(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                                     uint16_t *out_device);
/* Host-slice form with exactly the reference signature: `db` is a host array
 * of n reference-layout records, `out` a host array of n*31 uint16_t.  A slice
 * of an attached host array (iris_db_attach_host) runs on the resident copy.
 * A slice inside a read-only shared mapping of a regular file -- what the
 * participant and resolver walk (src/main.rs:386-391, 426-431; 455-460,
 * 511-516) -- runs on the device's copy of that file's records, made on first
 * use (read from the file in 256-MB granules, a call's missing ones and up to
 * 1 GB after them at once; a read that comes up short -- the file shrank --
 * drops the copy and the call uploads its slice) and kept.  Like the reference,
 * which maps the file once and treats it as immutable (src/main.rs:389; "Sync
 * from database" is a TODO at :402,415), the copy stands for the file as it was
 * read.  What every call re-checks: the file behind the mapping (device, inode,
 * size, mtime, ctime), so write(2), truncate, replace or rename-over, and a
 * mapping unmapped or replaced at the same address, drop the copy; the mapping's
 * file offset, at least every 200 ms; and three 64-byte snapshots of records in
 * the slice, which catch a change inside them whose timestamps did not move.
 * What it cannot see: stores through a writable MAP_SHARED mapping (this process's
 * or another's) into pages already dirty, which move no timestamp, outside the
 * three probed snapshots -- such records are served as they were read, for as
 * long as the copy lives.  A caller that changes its file that way calls
 * iris_device_drop_resident_range.  Copies are a cache: together at most
 * IRIS_RESIDENT_MAX_MB (default half the device), evicted least recently used
 * when a device allocation would fail, freed when their mapping is gone.  Files
 * that do not fit and IRIS_AUTO_RESIDENT=0 keep the upload path.  Any other
 * slice is uploaded (PCIe) and packed first. */
int iris_engine_batch_process_host(iris_engine_t *engine, const void *db, uint64_t n, uint16_t *out);
/* Frees the device's resident file copies (a failing iris_db_create does so too
 * before it retries); iris_config reports them as resident=count/bytes. */
int iris_device_drop_resident(iris_device_t *dev);
/* Frees the resident copy of the file mapping that holds host address ptr (of any
 * record kind), and forgets a refusal of that mapping: the next call on its slices
 * copies the file afresh.  For a caller that changed the file in a way the per-call
 * check does not see (stores through a writable shared mapping into pages already
 * dirty, see iris_engine_batch_process_host).  No copy there: nothing to do (0). */
int iris_device_drop_resident_range(iris_device_t *dev, const void *ptr);

/* Template engine, per template and rotation k: num = popcount((qp^ep)&qm&em),
 * den = popcount(qm&em) with q rotated by k-15 (src/template.rs:49-64).
 * num_out / den_out: host arrays of n*31 uint16_t (either may be NULL). */
int iris_template_counts(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                         uint16_t *num_out, uint16_t *den_out);
/* Template::distance(query, db[i]) for each i (src/template.rs:43-47):
 * out is a host array of n doubles (bit-exact to the reference). */
int iris_template_distances(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                            double *out);
/* Fused search: per-template distance + global min / argmin with the
 * resolver's strict-< lowest-index rule (src/main.rs:581-621).  Indices in
 * *out are global: db index + index_base.  dist_out_device (optional, may be
 * NULL) receives the n per-template distances in DEVICE memory. */
int iris_template_search(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                         uint64_t index_base, double *dist_out_device, iris_match_t *out);

/* Pipelined form of iris_template_search (no reference counterpart: the
 * reference's calls block, src/lib.rs:42-53): enqueues the search and returns
 * at once; iris_pending_wait blocks for THAT search only and frees the handle,
 * so the next query's search can be enqueued (and its engine built) while the
 * caller exchanges or consumes this result.  The engine may be destroyed
 * before the wait; the database must stay alive and unmodified until it.
 * Results and ordering are as before; a later search of the same records may be partly computed by an earlier pass. */
int iris_template_search_async(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                               uint64_t index_base, iris_pending_t **out);
int iris_pending_wait(iris_pending_t *pending, iris_match_t *out);

/* Batched queries (BASELINE configs[2]): nq query Templates searched against
 * one TILES template database in one pass; out[q] is query q's best match
 * (same rules as iris_template_search).  DB layout must be TILES, except for
 * nq <= 3, which runs as streaming passes over any layout. */
int iris_template_batch_engine_new(iris_device_t *dev, const iris_template_t *queries, uint32_t nq,
                                   iris_engine_t **out);
int iris_template_batch_search(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                               uint64_t index_base, iris_match_t *out);

/* Batched DistanceEngine (no reference counterpart: the reference builds one DistanceEngine per
 * query, src/lib.rs:33-52, and a participant with Q pending queries walks its share file Q
 * times): nq DistanceEngines at once, run against a share database in one pass.  On the TILES
 * layout every share tile is read once for up to four queries; on LANES the batch runs nq
 * single-query passes (the layout only selects the kernel family; results are identical).
 * Destroyed with iris_engine_destroy.  The single-query calls (iris_engine_batch_process*)
 * refuse a batch engine and these refuse a single-query one (IRIS_E_ARG). */
#define IRIS_DISTANCE_BATCH_MAX 64
/* nq DistanceEngines at once: queries = nq x 12800 u16 (EncodedBits), any values */
int iris_distance_batch_engine_new(iris_device_t *dev, const uint16_t *queries, uint32_t nq, iris_engine_t **out);
/* out[(q*n + i)*31 + k] = dot_u16(rot(queries[q], k-15), db[first+i])  -- query-major: slab q is exactly
 * what iris_engine_batch_process of a DistanceEngine(queries[q]) writes (src/lib.rs:42-52).  Host /
 * device output forms (out: host array, out_device: DEVICE array, of nq*n*31 uint16_t).  n == 0
 * writes nothing. */
int iris_distance_batch_process(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n, uint16_t *out);
int iris_distance_batch_process_device(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                                       uint16_t *out_device);

/* Batched MasksEngine and resolver step (no reference counterpart: the reference computes the
 * denominators and decodes one query at a time, src/main.rs:506-519 and 597-621, so a resolver with
 * Q pending queries reads its masks Q times): nq MasksEngines at once.  On the TILES layout ranges
 * past 1024 tiles of 32 records read every mask tile once for up to four queries; smaller ranges
 * and LANES databases run one single-query pass per query (results are identical).  Destroyed
 * with iris_engine_destroy.  The single-query calls (iris_engine_batch_process*,
 * iris_resolver_search_masks*) refuse a masks batch engine and these refuse a single-query or a
 * distance batch engine (IRIS_E_ARG). */
#define IRIS_MASKS_BATCH_MAX 64
/* nq MasksEngines at once: query_masks = nq x 200 u64 (Bits), any values */
int iris_masks_batch_engine_new(iris_device_t *dev, const uint64_t *query_masks, uint32_t nq, iris_engine_t **out);
/* out[(q*n + i)*31 + k] = dot_bool(rot(query_masks[q], k-15), db[first+i])  -- query-major: slab q is exactly
 * what iris_engine_batch_process of a MasksEngine(query_masks[q]) writes (src/lib.rs:69-79).  Host /
 * device output forms (out: host array, out_device: DEVICE array, of nq*n*31 uint16_t).  n == 0
 * writes nothing. */
int iris_masks_batch_process(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n, uint16_t *out);
int iris_masks_batch_process_device(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                                    uint16_t *out_device);
/* The fused resolver step (iris_resolver_search_masks, below) for all nq queries in one pass over
 * masks records [first, first+n): shares_device[p] is a DEVICE array of nq*n*31 uint16_t, query-major
 * -- exactly what iris_distance_batch_process_device wrote for participant p over the same range
 * (parts = 1..8).  out[q] (nq matches) is what iris_resolver_search_masks gives for
 * MasksEngine(query_masks[q]) and slab q of every part.  dist_out_device: NULL, or a DEVICE array of
 * nq*n doubles (query-major). */
int iris_resolver_batch_search_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                                     const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                     double *dist_out_device, iris_match_t *out);

/* ---------------------------------------------------------------- resolver
 * The resolver's aggregation (src/main.rs:597-621) fused on the GPU: for each
 * entry i, num = wrapping sum over the `parts` participants' [u16;31] shares,
 * decode_distance(num, denoms[i]) (src/lib.rs:97-107), then the first entry
 * with a strictly smaller distance.  out->index = index_base + i, out->num =
 * the decoded uneq count, out->den = the denominator.  At most 8 parts.
 * Device form: all arrays are DEVICE arrays of n*31 uint16_t.            */
int iris_resolver_search(iris_device_t *dev, const uint16_t *const *shares_device, uint32_t parts,
                         const uint16_t *denoms_device, uint64_t n, uint64_t index_base, double *dist_out_device,
                         iris_match_t *out);
/* The resolver step with the denominators computed on the fly: `engine` is
 * the MasksEngine of the query mask, records [first, first+n) of the masks
 * database give the denominators (MasksEngine::batch_process, never written
 * to memory on the TILES layout), shares_device[p] are DEVICE arrays of n*31
 * uint16_t with row i belonging to record first+i (src/main.rs:510-519 +
 * 597-621 in one pass).  Same result as iris_resolver_search over the
 * engine's output; indices are i + index_base. */
int iris_resolver_search_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                               const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                               double *dist_out_device, iris_match_t *out);
/* iris_resolver_search_masks with the participants' outputs in host memory (src/main.rs:510-519 +
 * 597-621: the rows as they arrive over the network; the reference's resolver computes the masks
 * denominators itself, here fused): shares[p] are host arrays of n x 31 u16, row i = record
 * first + i.  The parts are summed (wrapping u16) on the host while the previous chunk's sum is
 * copied and searched; blocking, one result; indices are i + index_base. */
int iris_resolver_search_masks_host(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                                    const uint16_t *const *shares, uint32_t parts, uint64_t index_base,
                                    iris_match_t *out);
/* Host form: shares[p] and denoms are host arrays, uploaded in chunks -- through the device's pinned
 * upload slots, overlapped with the kernels, or by the runtime's copy, whichever moved this
 * device's large host uploads faster lately (as for iris_db_write); blocking, one result. */
int iris_resolver_search_host(iris_device_t *dev, const uint16_t *const *shares, uint32_t parts,
                              const uint16_t *denoms, uint64_t n, uint64_t index_base, iris_match_t *out);

/* ------------------------------------------------------ threshold matching
 * Every record under a distance, in one database pass -- what a uniqueness check or an
 * identification asks for.  The reference keeps only the single best record: its loops
 * (src/template.rs:43-47 per record, src/main.rs:616-621 over records) fold a minimum, and the
 * calls below generalise those loops from "the minimum" to "all below a threshold".  The
 * threshold itself has no reference counterpart.
 *
 * A record matches iff distance < threshold, where distance is the f64 the sibling search call
 * (iris_template_search, iris_resolver_search, iris_resolver_search_masks) would report if that
 * record were the only one in the range: (double)num / (double)den of its best rotation (exact
 * fraction minimum, lowest rotation on ties; decode_distance of the wrapping share sum,
 * src/lib.rs:97-107, for the resolver forms).  The decision is that f64 comparison, bit for bit.
 * A record without a valid rotation (every den == 0, distance +inf) never matches, not even for
 * threshold = +inf.  threshold: any f64 but NaN (IRIS_E_ARG); <= 0 matches nothing, +inf every
 * record with a valid rotation.
 *
 * out: host array of cap iris_match_t; *count (required) receives the number of matches in the
 * range, which may exceed cap.  out receives the min(*count, cap) matches of lowest index, in
 * ascending index order, each filled as the sibling search would (reserved = 0); entries past them
 * are left untouched.  cap == 0 with out == NULL counts only.  n == 0 gives *count = 0.  The
 * result is deterministic: identical calls return identical bytes.  Argument, engine-kind and
 * range checks and locking are the sibling search's; a batch engine is refused (a masks batch
 * engine and a template batch engine have forms of their own, iris_resolver_batch_matches_masks
 * and iris_template_batch_matches below).
 *
 * The library keeps a per-device match buffer (never more than n records) and does not guess its
 * size: a pass that reports more matches than the buffer holds is run once more with the buffer
 * grown to the reported count.
 *
 * Out of scope: of the batch engines, the distance batch engine (its rows are shares, no
 * distances; the masks batch engine has iris_resolver_batch_matches_masks and the template batch
 * engine iris_template_batch_matches, both below); the host-array forms (*_host); device groups (a
 * variable-length exchange; iris_group_template_batch_search's sibling included); and, of the
 * asynchronous pipeline, every form but the single-query template one
 * (iris_template_matches_async, below: no resolver, batch-engine or group form). */
/* iris_template_search's sibling (src/template.rs:43-47 + src/main.rs:616-621): indices are
 * index_base + first + i. */
int iris_template_matches(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                          uint64_t index_base, double threshold,
                          iris_match_t *out, uint64_t cap, uint64_t *count);
/* iris_resolver_search's sibling (src/main.rs:597-621; the per-row minimum over rotations is
 * decode_distance's, the template.rs:43-47 fold): DEVICE arrays of n*31 uint16_t; indices are index_base + i. */
int iris_resolver_matches(iris_device_t *dev, const uint16_t *const *shares_device, uint32_t parts,
                          const uint16_t *denoms_device, uint64_t n, uint64_t index_base, double threshold,
                          iris_match_t *out, uint64_t cap, uint64_t *count);
/* iris_resolver_search_masks' sibling (src/main.rs:510-519 + 597-621; rotations folded as in
 * src/template.rs:43-47): indices are index_base + i, i the row within the range. */
int iris_resolver_matches_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                                const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                double threshold, iris_match_t *out, uint64_t cap, uint64_t *count);
/* iris_resolver_batch_search_masks' sibling, for a masks batch engine (iris_masks_batch_engine_new,
 * nq = 1..64): the threshold lists of all nq queries in one pass over masks records
 * [first, first+n) (src/main.rs:510-519 + 597-621 per query; rotations folded as in
 * src/template.rs:43-47).  The inputs are iris_resolver_batch_search_masks': shares_device[p] is
 * participant p's query-major DEVICE array of nq*n*31 uint16_t (parts = 1..8).  One threshold for
 * the whole batch.
 *
 * counts (required): host array of nq uint64_t; counts[q] is the exact number of matches of query
 * q in the range and may exceed cap.  out: host array of nq*cap iris_match_t, query-major;
 * out[q*cap + j], j < min(counts[q], cap), are query q's matches of lowest index in ascending index
 * order, each filled as iris_resolver_matches_masks fills it (index = index_base + row within the
 * range, reserved = 0); entries past a query's list are left untouched.  cap == 0 with out == NULL
 * counts only.  n == 0 sets every count to 0.
 *
 * Contract: query q's list and count are byte for byte what iris_resolver_matches_masks returns
 * for MasksEngine(query_masks[q]) with slab q of every part.  The decision is the same f64
 * comparison: a record whose every denominator is 0 never matches, not even under +inf;
 * threshold <= 0 matches nothing; NaN is refused (IRIS_E_ARG).  Identical calls return identical
 * bytes.  The value arguments (threshold, out / cap, counts, parts) are checked before the
 * handles; engine, database and range checks are iris_resolver_batch_search_masks'.
 *
 * On TILES ranges the batch kernel runs (past 1024 tiles) the masks are read once per group of up
 * to four queries; a query whose list does not fit its share of the device's match buffer has only
 * its own group (elsewhere: the query alone) run once more, so no query reads the masks more than
 * twice and the buffer never holds more than one group's records. */
int iris_resolver_batch_matches_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                                      const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                      double threshold, iris_match_t *out, uint64_t cap, uint64_t *counts);
/* iris_template_batch_search's sibling, for a template batch engine (iris_template_batch_engine_new,
 * any nq it accepts): the threshold lists of all nq queries in one pass over template records
 * [first, first+n) (src/template.rs:43-47 per record, src/main.rs:616-621 over records, per
 * query) -- many probes against one enrolled database, as a deduplication run asks.  One threshold
 * for the whole batch.
 *
 * counts (required): host array of nq uint64_t; counts[q] is the exact number of matches of query
 * q in the range and may exceed cap.  out: host array of nq*cap iris_match_t, query-major;
 * out[q*cap + j], j < min(counts[q], cap), are query q's matches of lowest index in ascending index
 * order, each filled as iris_template_matches fills it (index = index_base + first + i,
 * reserved = 0); entries past a query's list are left untouched.  cap == 0 with out == NULL counts
 * only.  n == 0 sets every count to 0.
 *
 * Contract: query q's list and count are byte for byte what iris_template_matches returns for
 * TemplateEngine(queries[q]) over the same range, index_base and threshold.  The decision is the
 * same f64 comparison on the best rotation (exact fraction, lowest rotation on ties): a record
 * without a valid rotation never matches, not even under +inf; threshold <= 0 matches nothing; NaN
 * is refused (IRIS_E_ARG).  Identical calls return identical bytes.  The value arguments
 * (threshold, out / cap, counts) are checked before the handles; engine, database, layout and
 * range checks are iris_template_batch_search's (more than 3 queries need a TILES database).
 *
 * More than 3 queries run one pass of the batched GEMM for all of them.  The first pass gives
 * every query room for min(n, max(1024, min(cap, 256 MiB / (24 nq)))) records of the device's match
 * buffer; a query whose list is longer has only its aligned block of 4 queries run once more, one
 * block at a time, so no query is computed more than twice and the buffer holds at most the first
 * pass's regions or one block's records.  Up to 3 queries run one single-query match pass each. */
int iris_template_batch_matches(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                                uint64_t index_base, double threshold,
                                iris_match_t *out, uint64_t cap, uint64_t *counts);

/* Pipelined form of iris_template_matches, as iris_template_search_async is of
 * iris_template_search (no reference counterpart: the reference's calls block, src/lib.rs:42-53;
 * the loops generalised are src/template.rs:43-47 + src/main.rs:616-621).  The submission
 * enqueues the pass and returns at once; iris_pending_matches_wait blocks for THAT pass only,
 * fills out (cap entries, the submission's cap; NULL only if cap == 0) and *count (required), and
 * frees the handle whatever it returns (but another submission's handle: see iris_pending_matches_t).
 *
 * Contract: out and *count are byte for byte what iris_template_matches(engine, db, first, n,
 * index_base, threshold, out, cap, count) would have returned at the submission: the exact total
 * even above cap, the min(*count, cap) matches of lowest index in ascending order, entries past
 * them untouched, n == 0 gives 0.  A pass that is still streaming the database may compute the
 * match pass submitted after it (same records of the same database, unwritten since; thresholds
 * may differ); the result does not depend on it.  A search never computes a match pass, nor the
 * reverse.
 *
 * Argument, engine-kind, range and NaN checks are iris_template_matches', made at the submission
 * (out and count at the wait); a batch engine is refused.  The engine may be destroyed before the
 * wait; the database must stay alive and unmodified until it.  Every pending holds device room
 * for min(n, max(cap, 1024)) records until its wait; a list longer than that room (cap > 0 only)
 * makes the wait run the pass once more, blocking. */
int iris_template_matches_async(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                                uint64_t index_base, double threshold, uint64_t cap,
                                iris_pending_t **out /* an iris_pending_matches_t */);
int iris_pending_matches_wait(iris_pending_t *pending /* an iris_pending_matches_t */, iris_match_t *out,
                              uint64_t *count);

/* ------------------------------------------------------------------- top-k
 * The k closest records of a range, best first, in one database pass -- the ranked candidate
 * list of rank-k identification, a review queue or threshold calibration, with no threshold
 * known in advance.  The reference has only the minimum: src/template.rs:43-47 per record, folded
 * over records by src/main.rs:616-621.  The calls below generalise that fold from "the first
 * record of the order" to "the first k"; k itself has no reference counterpart.
 *
 * The order is the sibling search's (iris_template_search, iris_resolver_search,
 * iris_resolver_search_masks): records are ordered by the exact fraction num/den of their best
 * rotation (u32 cross-multiplication, never a float), then by the lowest index; the best rotation
 * is the exact fraction minimum, lowest rotation on ties (decode_distance of the wrapping share
 * sum, src/lib.rs:97-107, for the resolver forms).  A record without a valid rotation (every
 * den == 0, distance +inf) is never listed.
 *
 * k: 1..IRIS_TOPK_MAX (IRIS_E_ARG otherwise).  out: host array of k iris_match_t; count
 * (required): *count = min(k, records of the range with a valid rotation).  out[0..*count) are
 * the first *count records of the order, best first, each filled as the sibling search fills its
 * one result (distance is the one IEEE division num/den, index = index_base + the sibling's
 * offset, num, den, rotation, reserved = 0); entries past *count are left untouched.  n == 0
 * gives *count = 0.  The order is total (indices are unique), so identical calls return identical
 * bytes.  It follows that out[0] is byte for byte the sibling search's result (*count == 0 where
 * the search reports +inf), that a call with k' < k returns the first k' entries of the call
 * with k, and that the entries below a threshold are the sibling *_matches list.
 *
 * The value arguments (k, out, count) are checked before the handles; engine-kind, database,
 * layout and range checks and the locking are the sibling search's; the single-query calls refuse
 * a batch engine (a masks batch engine has iris_resolver_batch_topk_masks and a template batch
 * engine iris_template_batch_topk, both below).  There is no dist_out_device.  The bytes copied
 * back per call are 24 k per query, whatever n is.
 *
 * Out of scope: of the batch engines, the distance batch engine (its rows are shares, no
 * distances; the masks batch engine has iris_resolver_batch_topk_masks and the template batch
 * engine iris_template_batch_topk); the host-array forms (*_host); the rest of the asynchronous pipeline
 * (the single-query template form has one, iris_template_topk_async below: no resolver, batch-engine
 * or group form); device groups (iris_topk_merge below is the hand-sharding answer) and k > 64. */
#define IRIS_TOPK_MAX 64
/* iris_template_search's sibling (src/template.rs:43-47 + src/main.rs:616-621): indices are
 * index_base + first + i. */
int iris_template_topk(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                       uint64_t index_base, uint32_t k, iris_match_t *out, uint32_t *count);
/* iris_resolver_search's sibling (src/main.rs:597-621; the per-row minimum over rotations is
 * decode_distance's, src/lib.rs:97-107): DEVICE arrays of n*31 uint16_t; indices are index_base + i. */
int iris_resolver_topk(iris_device_t *dev, const uint16_t *const *shares_device, uint32_t parts,
                       const uint16_t *denoms_device, uint64_t n, uint64_t index_base, uint32_t k,
                       iris_match_t *out, uint32_t *count);
/* iris_resolver_search_masks' sibling (src/main.rs:510-519 + 597-621): indices are
 * index_base + i, i the row within the range. */
int iris_resolver_topk_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                             const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                             uint32_t k, iris_match_t *out, uint32_t *count);
/* iris_resolver_batch_search_masks' sibling, for a masks batch engine (iris_masks_batch_engine_new,
 * nq = 1..64): the k closest records of every query in one pass over masks records
 * [first, first+n) (src/main.rs:510-519 + 597-621 per query; rotations folded as in
 * src/template.rs:43-47; k has no reference counterpart).  The inputs are
 * iris_resolver_batch_search_masks': shares_device[p] is participant p's query-major DEVICE array
 * of nq*n*31 uint16_t (parts = 1..8).  One k (1..IRIS_TOPK_MAX) for the whole batch.
 *
 * out: host array of nq*k iris_match_t, query-major; counts (required): host array of nq uint32_t,
 * counts[q] = min(k, records of the range with a valid rotation for query q).  out[q*k + j],
 * j < counts[q], are the first records of the search order, best first, each filled as
 * iris_resolver_topk_masks fills it (index = index_base + row within the range, reserved = 0);
 * entries past a query's count are left untouched.  n == 0 sets every count to 0.
 *
 * Contract: query q's list and count are byte for byte what iris_resolver_topk_masks returns for
 * MasksEngine(query_masks[q]) with slab q of every part.  It follows that out[q*k] is
 * iris_resolver_batch_search_masks' result for q, that a smaller k returns per-query prefixes and
 * that identical calls return identical bytes.  The value arguments (k, out, counts, parts) are
 * checked before the handles; engine, database and range checks are
 * iris_resolver_batch_search_masks'.  There is no dist_out_device.
 *
 * On TILES ranges the batch kernel runs (past 1024 tiles) the masks are read once per group of up
 * to four queries, every wave keeping one resident list per query; elsewhere each query runs
 * iris_resolver_topk_masks' own pass on its slab.  The call waits once and copies back 24 k bytes
 * per query. */
int iris_resolver_batch_topk_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                                   const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                   uint32_t k, iris_match_t *out, uint32_t *counts);
/* iris_template_batch_search's sibling, for a template batch engine (iris_template_batch_engine_new,
 * any nq it accepts): the k closest records of every query in one pass over template records
 * [first, first+n) (src/template.rs:43-47 per record, src/main.rs:616-621 over records, per query;
 * k has no reference counterpart) -- many probes against one enrolled database, each probe's ranked
 * candidates instead of its minimum alone.  One k (1..IRIS_TOPK_MAX) for the whole batch.
 *
 * out: host array of nq*k iris_match_t, query-major; counts (required): host array of nq uint32_t,
 * counts[q] = min(k, records of the range with a valid rotation for query q).  out[q*k + j],
 * j < counts[q], are the first records of the search order, best first, each filled as
 * iris_template_topk fills it (index = index_base + first + i, reserved = 0); entries past a
 * query's count are left untouched.  n == 0 sets every count to 0 and writes nothing else.
 *
 * Contract: query q's list and count are byte for byte what iris_template_topk returns for
 * TemplateEngine(queries[q]) over the same range and index_base.  It follows that, where
 * counts[q] > 0, out[q*k] is iris_template_batch_search's result for q, that a smaller k returns
 * per-query prefixes and that identical calls return identical bytes.  The value arguments (k, out,
 * counts) are checked before the handles; engine, database, layout and range checks are
 * iris_template_batch_search's (more than 3 queries need a TILES database).  There is no
 * dist_out_device.
 *
 * More than 3 queries run one pass of the batched GEMM for all of them: a workgroup of 8 waves holds
 * 2 queries x 16 tiles (2 x 2 per wave), G workgroups share a query group, and every wave keeps one
 * resident sorted list per query of its own across its N-groups -- 8 G lists of k records a query,
 * folded 64 lists at a time by the merge levels for all queries together.  The lists take
 * nqp (8 G + ceil(8 G / 64)) k records of the device's match buffer (nqp: nq padded to 4); top-k
 * always fits, so no pass runs twice.  Up to 3 queries run iris_template_topk's own pass each.  The
 * call waits once and copies back 24 k bytes per query. */
int iris_template_batch_topk(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                             uint64_t index_base, uint32_t k, iris_match_t *out, uint32_t *counts);
/* Host only, no device: merges top-k lists (of shards, chunks, GPUs) that carry global indices
 * into one -- the top-k counterpart of iris_match_merge, src/main.rs:616-621 generalised to k.
 * The same order over nrecords records; records with den == 0 or index == UINT64_MAX are
 * ignored; two records with the same index are a caller error (IRIS_E_ARG).  out (k records,
 * not overlapping `records`) receives *count = min(k, valid records) records, best first, copied
 * as given; entries past *count are left untouched. */
int iris_topk_merge(const iris_match_t *records, uint64_t nrecords, uint32_t k, iris_match_t *out, uint32_t *count);

/* Pipelined form of iris_template_topk, as iris_template_search_async is of iris_template_search
 * and iris_template_matches_async of iris_template_matches (no reference counterpart: the
 * reference's calls block, src/lib.rs:42-53; the loops generalised are src/template.rs:43-47 +
 * src/main.rs:616-621).  The submission enqueues the pass and returns at once;
 * iris_pending_topk_wait blocks for THAT pass only, fills out (k entries, the submission's k;
 * required) and *count (required), and frees the handle whatever it returns (but a handle of
 * another submission: see iris_pending_topk_t).
 *
 * Contract: out[0..*count) and *count are byte for byte what iris_template_topk(engine, db, first,
 * n, index_base, k, out, count) would have returned at the submission; entries past *count are
 * untouched, n == 0 gives 0.  A pass that is still streaming the database may compute the top-k
 * pass submitted after it (same records of the same database, unwritten since; k may differ); the
 * result does not depend on it.  A top-k pass computes neither a search nor a match pass, nor the
 * reverse.
 *
 * The value arguments (k in 1..IRIS_TOPK_MAX, out) are checked before the handles; engine-kind,
 * database, layout and range checks are iris_template_topk's, made at the submission (the wait's
 * out and count at the wait); a batch engine is refused, and so is an engine that keeps no host
 * copy of its query.  The engine may be destroyed before the wait; the database must stay alive
 * and unmodified until it.  Every pending holds one list of k records per wave of its pass (24 k
 * bytes each; 120 MB at k = 64 over 10M templates) until its wait. */
int iris_template_topk_async(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                             uint64_t index_base, uint32_t k, iris_pending_t **out /* an iris_pending_topk_t */);
int iris_pending_topk_wait(iris_pending_t *pending /* an iris_pending_topk_t */, iris_match_t *out,
                           uint32_t *count);

/* -------------------------------------------------------------- histograms
 * The distribution of a range's distances in one database pass -- the impostor score histogram a
 * false-match rate is read from, and so the answer to where a threshold belongs before
 * iris_template_matches can use one.  The reference has no counterpart; the loops generalised are
 * the search's: src/template.rs:43-47 per record, src/main.rs:616-621 over records, with "count it
 * in its bin" in place of "keep the minimum".
 *
 * Distance: a record's distance is the f64 the sibling search would report if that record were
 * alone in the range, (double)num / (double)den of its best rotation (exact fraction minimum,
 * lowest rotation on ties).  Binning: a record with a valid rotation is counted in bin
 * min(nbins - 1, floor(distance * nbins)), so bin j covers [j/nbins, (j+1)/nbins) and the last bin
 * also takes distance 1.0.  A record without a valid rotation (every den == 0, distance +inf) is
 * counted in *invalid and in no bin: sum(bins) + *invalid == n, always.
 *
 * nbins: a power of two in 1..IRIS_HIST_MAX_BINS (IRIS_E_ARG otherwise).  A power of two makes
 * distance * nbins exact in f64, and two things follow:
 *   1. the prefix sum bins[0] + ... + bins[j-1] equals, exactly, the total iris_template_matches
 *      reports for threshold = (double)j / nbins over the same range;
 *   2. the bin equals the integer floor(num * nbins / den) (the product stays below 2^24), which
 *      is what the device computes: no f64 division per record.
 *
 * bins (nbins uint64_t) and invalid are required host pointers.  The call OVERWRITES them, it does
 * not accumulate: histograms of chunks, shards or GPUs add, so a caller sums them itself.  n == 0
 * writes zeros; a refused call leaves both untouched.  Counts are integers and their sum does not
 * depend on the order of the additions, so identical calls return identical bytes.
 *
 * The value arguments (nbins, bins, invalid) are checked before the handles; engine-kind,
 * database, layout and range checks and the locking are the sibling search's.  The single-query
 * call refuses a batch engine; the batch call has iris_template_batch_matches' checks (more than 3
 * queries need a TILES database).  The bytes copied back per call are 8 (nbins + 1) per query,
 * whatever n is.
 *
 * The pipelined form of the single-query template call is iris_template_report_async with
 * parts = IRIS_REPORT_HIST (section "pipelined reports" below).
 *
 * Out of scope: pipelined resolver and batch-engine forms and the device-group forms (histograms
 * add: a caller sums its shards); host-array forms; bin counts that are not a power of two and caller-given edges;
 * weighted counts; more than 1024 bins (the batched kernel keeps four queries' histograms in LDS
 * beside its 128-KiB fragment ring: 16 KiB at 1024 bins fit the CU's 160 KiB, 64 KiB at 4096 do
 * not). */
#define IRIS_HIST_MAX_BINS 1024u
/* iris_template_search's sibling: the distribution of the distances that search folds a minimum of */
int iris_template_histogram(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                            uint32_t nbins, uint64_t *bins /* [nbins] */, uint64_t *invalid);
/* iris_template_batch_search's sibling, for a template batch engine: one histogram per query in
 * one pass.  bins: nq*nbins uint64_t, query-major; invalid: nq uint64_t.  Contract: histogram q and
 * invalid[q] are byte for byte what iris_template_histogram returns for TemplateEngine(queries[q])
 * over the same range.  More than 3 queries run one pass of the batched GEMM, every workgroup
 * keeping its queries' histograms in LDS across its walk; up to 3 run iris_template_histogram's own
 * pass each.  The call waits once. */
int iris_template_batch_histogram(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                                  uint32_t nbins, uint64_t *bins /* [nq][nbins] */, uint64_t *invalid /* [nq] */);

/* --------------------------------------------------------- combined passes
 * The match list, the k closest records and the distance histogram of ONE probe from ONE read of
 * the range.  An identification service asks all three for the same probe -- the list is the
 * decision, the neighbours go to the operator and the audit log, the histogram shows whether the
 * scores still sit where the threshold was calibrated -- and each sibling call is a full pass over
 * the database that is bound by reading it.  All three are functions of the one value the search's
 * loops produce per record, its best rotation (src/template.rs:43-47 per record,
 * src/main.rs:616-621 over records): a report pass computes it once and feeds every selected sink.
 *
 * report->parts selects the parts, IRIS_REPORT_* bits: at least one, no others (IRIS_E_ARG).  EACH
 * SELECTED PART IS BYTE FOR BYTE WHAT ITS SIBLING CALL WRITES for the same engine, database,
 * range, index_base and arguments:
 *   MATCHES  matches[0 .. min(matches_count, matches_cap)) and matches_count are
 *            iris_template_matches' out and *count for (threshold, cap);
 *   TOPK     topk[0 .. topk_count) and topk_count are iris_template_topk's out and *count for k;
 *   HIST     bins[0 .. nbins) and invalid are iris_template_histogram's for nbins.
 * That sentence is the whole semantics: thresholds are decided on the f64 the search would report,
 * order is the exact fraction and then the lowest index, the bin is the integer num * nbins / den,
 * and a record without a valid rotation is in no list and counts in `invalid`.  The fields and
 * arrays of a part that is not selected are neither read nor written.
 *
 * Refusals: the value arguments are checked before the handles -- parts, then each selected part's
 * own arguments under its sibling's rules (a NaN threshold, matches NULL with a cap, k outside
 * 1..IRIS_TOPK_MAX, topk NULL, nbins not a power of two in 1..IRIS_HIST_MAX_BINS, bins NULL) -- then
 * the engine, the database and the range as in the siblings: a single-query template engine and a
 * templates database of either layout; a batch engine is IRIS_E_ARG.  A refused or failed call
 * writes nothing, the out fields of the struct included: nothing is written before every selected
 * part has succeeded.  n == 0: the counts and the bins are zero, and nothing is launched.
 *
 * One part selected runs that sibling's own pass.  Two or three run one pass, followed on the
 * stream by the top-k merge and the histogram's reduce, and the call waits once; a match list that
 * overflows the room of the first pass runs the matches part alone once more, as
 * iris_template_matches does (never with matches_cap == 0).
 *
 * The pipelined template report is iris_template_report_async (section "pipelined reports" below):
 * there a running report pass serves the next one; this blocking call neither hosts nor is hosted.
 *
 * Out of scope: pipelined resolver and batch-engine reports;
 * template batch engines here (iris_template_batch_report, section "template batch reports" below,
 * is their call) and masks batch engines; host-array forms and
 * device groups; more than one threshold, k or histogram per call; a search part -- topk[0] at
 * k = 1 is the search's result.  The resolver forms, iris_resolver_report and
 * iris_resolver_report_masks, take this struct and these bits: section "resolver reports" below. */
#define IRIS_REPORT_MATCHES 1
#define IRIS_REPORT_TOPK 2
#define IRIS_REPORT_HIST 4
typedef struct iris_report {
    uint32_t parts;         /* in: IRIS_REPORT_* bits, at least one, no others */
    uint32_t k;             /* in, TOPK: 1..IRIS_TOPK_MAX */
    uint32_t nbins;         /* in, HIST: a power of two, 1..IRIS_HIST_MAX_BINS */
    uint32_t topk_count;    /* out, TOPK */
    double threshold;       /* in, MATCHES: not NaN */
    iris_match_t *matches;  /* in, MATCHES: room for matches_cap records (may be NULL when the cap is 0) */
    uint64_t matches_cap;   /* in, MATCHES */
    uint64_t matches_count; /* out, MATCHES: the exact total, also when it exceeds the cap */
    iris_match_t *topk;     /* in, TOPK: room for k records */
    uint64_t *bins;         /* in, HIST: nbins words */
    uint64_t invalid;       /* out, HIST */
} iris_report_t;
/* report: the caller's iris_report_t.  It crosses as void *: the functions of this header take
 * scalars, opaque handles and the two value structs iris_match_t and iris_template_t, the closed set
 * every binding mirrors, and a struct of arguments is memory the caller lays out as above. */
int iris_template_report(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                         uint64_t index_base, void *report /* iris_report_t * */);

/* -------------------------------------------------------- pipelined reports
 * Pipelined form of iris_template_report, as iris_template_topk_async is of iris_template_topk (no
 * reference counterpart: the reference's calls block, src/lib.rs:42-53; the loops generalised are
 * src/template.rs:43-47 + src/main.rs:616-621).  A service that runs a query stream gets the match
 * list, the k closest records and the histogram of every probe from one shared pass: a report pass
 * that is still streaming the database also computes the report pass submitted after it.
 *
 * Submission: reads only the in scalars of *report -- parts, threshold, matches_cap, k, nbins --
 * and copies them; it does not read the array pointers and writes nothing to the struct.  It
 * enqueues the pass and returns at once.  The value arguments are refused before the handles under
 * iris_template_report's rules: report NULL, parts, then each selected part's scalars (a NaN
 * threshold, k outside 1..IRIS_TOPK_MAX, nbins not a power of two in 1..IRIS_HIST_MAX_BINS); the
 * pointer checks move to the wait.  Then out == NULL, then the engine, database, layout and range
 * as iris_template_report checks them; a batch engine is refused, and so is an engine that keeps
 * no host copy of its query.  A refused submission leaves *out alone.
 *
 * Wait: iris_pending_report_wait takes the caller's iris_report_t.  Its parts must equal the
 * submission's, and so must matches_cap, k and nbins of the selected parts (IRIS_E_ARG naming the
 * field otherwise: the arrays' sizes follow from them); threshold is not read.  The pointers of
 * the selected parts are checked under the sibling rules (matches may be NULL only with a cap of
 * 0; topk and bins are required).  It blocks for THAT pass only, writes the out fields and arrays
 * of the selected parts, and frees the handle whatever it returns -- a failed check included --
 * but a handle of another kind of submission is refused with both names and left alone.
 *
 * Contract: each selected part is byte for byte what iris_template_report would have written at the
 * submission for the same arguments, and so what iris_template_matches, iris_template_topk and
 * iris_template_histogram write; entries past the counts are untouched; fields and arrays of
 * unselected parts are neither read nor written; nothing is written before every selected part has
 * succeeded (the histogram's "sums to n" check and a match list's second pass included).  n == 0
 * gives zero counts and zero bins, launches nothing, and the handle owns no event or buffers.  A
 * match list longer than the pass's room (max(matches_cap, 1024) records; never with a cap of 0)
 * runs the matches part alone once more at the wait, blocking.
 *
 * Sharing: a report pass hosts only a report pass and is hosted only by one (same records of the
 * same database, unwritten since; one guest per pass); the two may differ in parts, threshold, cap,
 * k and nbins, and the result does not depend on it.  A handle of this call is a report pass
 * whatever parts holds: parts = IRIS_REPORT_HIST is the pipelined histogram.  Kernel stat
 * "report_shared": registrations and tile groups carried.
 *
 * The engine may be destroyed before the wait; the database must stay alive and unmodified until
 * it.  Until its wait a pending holds one device buffer: the three sinks (128 bytes), the
 * histogram's 64 copies of nbins + 1 counters (525 KB at 1024 bins), 24 bytes per record of the
 * match list's room (24 KB at caps up to 1024) and one list of k records per wave of its pass
 * (120 MB at k = 64 over 10M templates, 1.9 MB at k = 1), and 10 KB of pinned host memory.
 *
 * Out of scope: resolver, batch-engine and device-group pipelines; a report pass hosting a search,
 * match or top-k pass, or the reverse; more than one guest per pass; k > 64. */
int iris_template_report_async(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                               uint64_t index_base, const void *report /* const iris_report_t * */,
                               iris_pending_t **out /* an iris_pending_report_t */);
int iris_pending_report_wait(iris_pending_t *pending /* an iris_pending_report_t */,
                             void *report /* iris_report_t * */);

/* ----------------------------------------------------- resolver histograms
 * The same distribution where the MPC deployment first has distances: at the resolver, after the
 * participants' [u16; 31] share rows are summed and decoded against the masks denominators
 * (src/main.rs:597-621, src/lib.rs:97-107).  Three calls, siblings of the three resolver search
 * calls with exactly their inputs; there is no index_base, no dist_out and no threshold, because a
 * histogram has no indices.  The contract is the histograms' above, restated for the resolver's
 * value range:
 *
 * A record is counted in bin min(nbins - 1, floor(distance * nbins)) of the f64 distance the
 * sibling search / matches call reports for it: the best rotation of uneq / den, in exact fraction
 * order, lowest rotation on ties.  A record whose 31 denominators are all zero is counted in
 * *invalid alone: sum(bins) + *invalid == n, always.  Garbage shares are not an error: uneq can be
 * up to 32767 and, in iris_resolver_histogram, den up to 65535, so a distance can exceed 1; such a
 * record falls in the last bin, by the same min.  The device bins in integers,
 * min(nbins - 1, num * nbins / den) with num * nbins <= 32767 * 1024 < 2^25 in u32, which equals
 * the f64 rule for every den in 1..65535.
 *
 * nbins: a power of two in 1..IRIS_HIST_MAX_BINS.  The prefix sum of j < nbins bins equals the
 * total the sibling *_matches* call reports for threshold = (double)j / nbins, cap = 0; the sum of
 * all bins is its total at +inf.  bins and invalid are OVERWRITTEN, never accumulated; n == 0
 * writes zeros; a refused call leaves both untouched; identical calls return identical bytes.
 * The value arguments (nbins, NULL outputs, parts 1..8) are checked before the handles; the other
 * checks and the locking are the sibling search's.
 *
 * Out of scope: host-array forms (*_host); pipelined and device-group forms; the distance batch
 * engine; other bin counts or caller-given edges; more than 1024 bins. */
/* iris_resolver_search's sibling: denominators given */
int iris_resolver_histogram(iris_device_t *dev, const uint16_t *const *shares_device, uint32_t parts,
                            const uint16_t *denoms_device, uint64_t n,
                            uint32_t nbins, uint64_t *bins /* [nbins] */, uint64_t *invalid);
/* iris_resolver_search_masks' sibling: the denominators computed on the fly from the masks
 * database (TILES: one fused pass; LANES: the masks kernel into a workspace, then the resolver's) */
int iris_resolver_histogram_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                                  const uint16_t *const *shares_device, uint32_t parts,
                                  uint32_t nbins, uint64_t *bins /* [nbins] */, uint64_t *invalid);
/* iris_resolver_batch_search_masks' sibling, for a masks batch engine (nq = 1..64) and query-major
 * share arrays: one histogram per query, up to 4 queries a masks pass.  Row q and invalid[q] are
 * byte for byte what iris_resolver_histogram_masks returns for MasksEngine(qmasks[q]) on slab q.
 * The call waits once. */
int iris_resolver_batch_histogram_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                                        const uint16_t *const *shares_device, uint32_t parts,
                                        uint32_t nbins, uint64_t *bins /* [nq][nbins] */, uint64_t *invalid /* [nq] */);

/* -------------------------------------------------------- resolver reports
 * The combined pass where the MPC deployment first has distances: at the resolver, after the
 * participants' [u16; 31] share rows are summed and decoded against the masks denominators
 * (src/main.rs:597-621, src/lib.rs:97-107).  No party holds templates there, so the resolver
 * operator who wants the match list, the k closest records and the score histogram of one probe
 * pays three passes over 1786 B per record (3 parts); a resolver report reads them once.  Both calls
 * take the iris_report_t and the IRIS_REPORT_* bits of "combined passes" unchanged.
 *
 * The whole semantics: EACH SELECTED PART IS BYTE FOR BYTE WHAT ITS SIBLING CALL WRITES for the
 * same inputs --
 *             iris_resolver_report         iris_resolver_report_masks
 *   MATCHES   iris_resolver_matches        iris_resolver_matches_masks      (threshold, cap, index_base)
 *   TOPK      iris_resolver_topk           iris_resolver_topk_masks         (k, index_base)
 *   HIST      iris_resolver_histogram      iris_resolver_histogram_masks    (nbins)
 * so indices are index_base + row, a distance above 1 from garbage shares joins the last bin, and
 * a record whose 31 denominators are all zero is in no list and counts in `invalid`.  The fields
 * and arrays of a part that is not selected are neither read nor written.
 *
 * Refusals: the value arguments are checked before the handles -- report->parts, then each selected
 * part's own arguments under its sibling's rules, then the number of share parts (1..8) -- then the
 * handles and the range as in the siblings: iris_resolver_report_masks needs a single-query masks
 * engine and a masks database of either layout; a masks batch engine is IRIS_E_ARG.  A refused or
 * failed call writes nothing, the out fields of the struct included.  n == 0: the counts and the
 * bins are zero, and nothing is launched.
 *
 * One part selected runs that sibling's own pass.  Two or three run one pass -- TILES: the fused
 * masks kernel; LANES and iris_resolver_report: the resolver kernel, for a masks database behind
 * the masks kernel into the workspace -- followed on the stream by the top-k merge and the
 * histogram's reduce, and the call waits once.  A match list that overflows the room of the first
 * pass runs the matches part alone once more (never with matches_cap == 0); on a LANES database
 * that pass reuses the denominators already in the workspace.
 *
 * Out of scope: the batch engines here (the masks batch engine has its report,
 * iris_resolver_batch_report_masks, section "masks batch reports" below, with per-slot sinks and a
 * per-group overflow rerun; the template batch engine has iris_template_batch_report, section
 * "template batch reports" below); host-array forms (*_host); pipelined forms; device groups; more than one
 * threshold, k or histogram per call; a search part -- topk[0] at k = 1 is the search's result. */
/* iris_resolver_search's sibling: denominators given */
int iris_resolver_report(iris_device_t *dev, const uint16_t *const *shares_device, uint32_t parts,
                         const uint16_t *denoms_device, uint64_t n, uint64_t index_base,
                         void *report /* iris_report_t * */);
/* iris_resolver_search_masks' sibling: the denominators computed on the fly from the masks database */
int iris_resolver_report_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                               const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                               void *report /* iris_report_t * */);

/* -------------------------------------------------- template batch reports
 * The combined pass of a template batch engine: every probe's match list, k closest records and
 * distance histogram from ONE GEMM pass over the range.  A deduplication run asks all three for
 * each of its probes, and each sibling batch call is a full GEMM that is bound by MFMA issue and
 * operand expansion, not by what happens to a record's best rotation at the end; a batch report
 * computes the best rotation once per (probe, record) and feeds every selected sink.
 *
 * report->parts selects the parts, the IRIS_REPORT_* bits of "combined passes": at least one, no
 * others, and reserved is 0 (IRIS_E_ARG).  One threshold, cap, k and bin count serve all nq queries
 * of the engine.  The whole semantics: EACH SELECTED PART IS BYTE FOR BYTE WHAT ITS SIBLING CALL
 * WRITES for the same engine, database, range, index_base and arguments --
 *   MATCHES  matches [nq][matches_cap] and matches_counts [nq] are iris_template_batch_matches' out
 *            and counts for (threshold, cap);
 *   TOPK     topk [nq][k] and topk_counts [nq] are iris_template_batch_topk's out and counts for k;
 *   HIST     bins [nq][nbins] and invalid [nq] are iris_template_batch_histogram's for nbins
 * -- and so, by those calls' contracts, what the single-query calls (and iris_template_report)
 * return per query.  Entries past a count stay untouched.  The fields and arrays of a part that is
 * not selected are neither read nor written.
 *
 * Refusals: the value arguments are checked before the handles -- parts and reserved, then each
 * selected part's own arguments under its sibling's rules, the per-query count arrays required --
 * then the engine, the database and the range as in the siblings: a batched template engine; more
 * than 3 queries need a TILES database.  A refused or failed call writes nothing: nothing is
 * written before every selected part has succeeded (an engine of up to 3 queries: the counts and
 * the invalid words not before every query has, a query's lists and bins not before every selected
 * part of that query has).  n == 0: the counts and the bins are zero, and nothing is launched.
 *
 * One part selected runs that sibling batch call.  Engines of up to 3 queries run one single-query
 * report per query (either layout), waiting once per query.  Otherwise two or three parts run one
 * GEMM pass for all queries, followed on the stream by the top-k merge levels of all queries, and
 * the call waits once; a query whose match list overflows the room of the first pass has its
 * aligned block of 4 queries run once more as iris_template_batch_matches' pass (never with
 * matches_cap == 0).
 *
 * Out of scope: the masks batch engine here (its report is iris_resolver_batch_report_masks,
 * section "masks batch reports" below, which takes this struct); pipelined, host-array and
 * device-group forms; per-query thresholds, k or bin counts; a search part -- topk[q][0] at k = 1
 * is query q's search result. */
typedef struct iris_batch_report {
    uint32_t parts;            /* in: IRIS_REPORT_* bits, at least one, no others */
    uint32_t k;                /* in, TOPK: 1..IRIS_TOPK_MAX */
    uint32_t nbins;            /* in, HIST: a power of two, 1..IRIS_HIST_MAX_BINS */
    uint32_t reserved;         /* in: 0 */
    double threshold;          /* in, MATCHES: not NaN */
    iris_match_t *matches;     /* in, MATCHES: [nq][matches_cap], may be NULL when the cap is 0 */
    uint64_t matches_cap;      /* in, MATCHES */
    uint64_t *matches_counts;  /* in, MATCHES: [nq], written: the exact totals */
    iris_match_t *topk;        /* in, TOPK: [nq][k] */
    uint32_t *topk_counts;     /* in, TOPK: [nq], written */
    uint64_t *bins;            /* in, HIST: [nq][nbins] */
    uint64_t *invalid;         /* in, HIST: [nq] */
} iris_batch_report_t;
/* report: the caller's iris_batch_report_t; it crosses as void *, as iris_template_report's does */
int iris_template_batch_report(iris_engine_t *engine, const iris_db_t *db, uint64_t first, uint64_t n,
                               uint64_t index_base, void *report /* iris_batch_report_t * */);

/* ------------------------------------------------------ masks batch reports
 * The combined pass of a masks batch engine at the resolver: every probe's match list, k closest
 * records and score histogram from ONE pass over the masks database and the participants' share
 * slabs (src/main.rs:597-621, src/lib.rs:97-107).  A resolver that batches its requests asks all
 * three of every probe, and each sibling batch call is a full pass; all three are functions of the
 * one value the fused resolver step holds per (query, record), the best rotation as exact integers.
 *
 * The call takes iris_batch_report_t and the IRIS_REPORT_* bits unchanged: report->parts selects
 * the parts (at least one, no others; reserved is 0), and one threshold, cap, k and bin count
 * serve all nq queries.  Every other input is iris_resolver_batch_search_masks': a masks batch
 * engine (nq = 1..64), a masks database of either layout, and the participants' query-major share
 * arrays (shares_device[p]: nq slabs of n rows of 31 u16, 2-byte aligned).  The whole semantics:
 * EACH SELECTED PART IS BYTE FOR BYTE WHAT ITS SIBLING BATCH CALL WRITES for the same arguments --
 *   MATCHES  matches [nq][matches_cap] and matches_counts [nq] are iris_resolver_batch_matches_masks'
 *            out and counts for (threshold, cap, index_base);
 *   TOPK     topk [nq][k] and topk_counts [nq] are iris_resolver_batch_topk_masks' out and counts
 *            for (k, index_base);
 *   HIST     bins [nq][nbins] and invalid [nq] are iris_resolver_batch_histogram_masks' for nbins
 * -- and so, by those calls' contracts, what the single-query *_masks calls (and
 * iris_resolver_report_masks) write on slab q.  Indices are index_base + row; a distance above 1
 * from garbage shares joins the last bin; a record whose 31 denominators are all zero (den == 0)
 * is in no list and counts in `invalid`.  Entries past a count stay untouched.  The fields and
 * arrays of a part that is not selected are neither read nor written.
 *
 * Refusals: the value arguments are checked before the handles -- report NULL, parts and reserved,
 * then each selected part's own arguments under its sibling's rules, then the number of share
 * parts (1..8) -- then the engine, the share pointers and the range as in the siblings: a masks
 * batch engine (a single-query masks engine is IRIS_E_ARG: iris_resolver_report_masks), a masks
 * database, and share pointers that are neither NULL nor at an odd address.  A refused or failed call writes nothing: nothing is written before every selected
 * part of every query has succeeded.  n == 0: the counts and the bins are zero, and
 * nothing is launched.
 *
 * One part selected runs that sibling batch call.  Two or three parts split the queries as the
 * siblings do: on TILES ranges the batch kernel runs, groups of 2..4 queries take one pass each of
 * the batch kernel's report form, a single left-over query the single-query report pass on its
 * slab; smaller TILES ranges and LANES databases run one single-query report pass per query.  Every
 * pass, each followed by its top-k merge, and one histogram reduce over all queries are enqueued
 * before the call waits once.  A query whose match list overflows the room of the first pass has
 * its group alone run once more as iris_resolver_batch_matches_masks' pass (never with
 * matches_cap == 0); the buffer then grows so that the next identical call is one pass.
 *
 * Out of scope: host-array (*_host), pipelined and device-group forms; per-query thresholds, k or
 * bin counts; a search part -- topk[q][0] at k = 1 is query q's iris_resolver_batch_search_masks
 * result; the distance batch engine; a K-split batch kernel for small ranges. */
int iris_resolver_batch_report_masks(iris_engine_t *engine, const iris_db_t *masks_db, uint64_t first, uint64_t n,
                                     const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                     void *report /* iris_batch_report_t * */);

/* ------------------------------------------------------------ arch plugin
 * The reference's backend plugin point (src/arch/mod.rs:5):
 *   dot_bool(&[u64;200], &[u64;200]) -> u16   src/arch/generic.rs:4-9
 *   dot_u16(&[u16;12800], &[u16;12800]) -> u16 src/arch/generic.rs:11-16
 * Batched all-pairs form (the criterion shapes of src/arch/mod.rs:29,53):
 * out[j*na + i] = dot(a[i], b[j]) for i < na, j < nb. */
int iris_dot_bool_batch(iris_device_t *dev, const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb,
                        uint16_t *out);
int iris_dot_u16_batch(iris_device_t *dev, const uint16_t *a, uint64_t na, const uint16_t *b, uint64_t nb,
                       uint16_t *out);

/* ------------------------------------------------- host-side value helpers
 * CPU implementations of the value-type operations the engines are built
 * from; they need no GPU. */
/* Bits::rotated (src/bits.rs:18-29,178-205): out[row,col] = in[row,(col-amount) mod 200] */
int iris_bits_rotated(const uint64_t in[IRIS_LIMBS], int32_t amount, uint64_t out[IRIS_LIMBS]);
/* EncodedBits::rotated (src/encoded_bits.rs:40-58) */
int iris_encoded_rotated(const uint16_t in[IRIS_BITS], int32_t amount, uint16_t out[IRIS_BITS]);
/* encode(&Template) (src/lib.rs:16-26): mask - 2*(pattern&mask) per bit as u16 */
int iris_encode(const iris_template_t *t, uint16_t out[IRIS_BITS]);
/* decode_distance(&[u16;31], &[u16;31]) -> f64 (src/lib.rs:97-107) */
int iris_decode_distance(const uint16_t distances[IRIS_ROTATIONS], const uint16_t denominators[IRIS_ROTATIONS],
                         double *out);
/* Diagnostics for the query tables an engine builds on the device
 * (iris_query.hip): iris_engine_query_tables copies an engine's rotated-query
 * table and MFMA fragments to the host; iris_host_query_tables builds the same
 * bytes with the host reference builders.  kind = IRIS_KIND_*; for
 * IRIS_KIND_TEMPLATES nq = 0 is a single-query engine and nq >= 4 the tiles of
 * a batched engine of nq queries (`query` = nq templates; `tab` unused).  The
 * sizes must be the layout's exactly (IRIS_E_ARG otherwise; see
 * iris_query_table_sizes). */
int iris_query_table_sizes(int kind, uint32_t nq, size_t *tab_bytes, size_t *frag_bytes);
int iris_engine_query_tables(const iris_engine_t *engine, void *tab, size_t tab_bytes, void *frag,
                             size_t frag_bytes);
int iris_host_query_tables(int kind, const void *query, uint32_t nq, void *tab, size_t tab_bytes, void *frag,
                           size_t frag_bytes);
/* Merges per-shard search results into the global one (min fraction, then
 * lowest index) — the cross-shard step of the resolver's argmin (src/main.rs:616-621). */
int iris_match_merge(const iris_match_t *records, uint64_t count, iris_match_t *out);

/* ------------------------------------------------------- device groups (multi-GPU)
 * The reference fans a query out to its participants and folds their answers
 * with a sequential strict-< minimum (src/main.rs:486-504, 616-621).  Here a
 * template database is split into contiguous shards across the gfx950 devices
 * of a group — shard s of S holds global records [s*N/S, (s+1)*N/S) — every
 * device searches its own shards with no data-path communication, and the
 * per-shard winners (24 B each, global indices) are exchanged with one RCCL
 * ncclAllGather over xGMI (librccl from /opt/rocm) and merged on every device
 * (exact fraction, then the lowest global index).
 *
 * Two ways to form a group:
 *  - iris_group_create: ONE process drives `n` devices (ncclCommInitAll's form:
 *    one id, every device a rank, created inside one RCCL group).
 *  - iris_group_create_rank: one device per process (e.g. a torchrun rank):
 *    rank 0 calls iris_group_unique_id and hands the 128 id bytes to every
 *    rank (any side channel); each rank then calls iris_group_create_rank with
 *    the same id.  Every rank makes the same group calls (SPMD); each holds
 *    and fills only its own shards.
 * Forming a group is bounded: RCCL's init (which blocks until every rank has
 * arrived) runs on a helper thread waited for at most IRIS_GROUP_TIMEOUT_MS
 * (default 120 s); if a peer never arrives the call fails (IRIS_E_HIP) instead
 * of hanging, the pending init is abandoned (it aborts its communicators should
 * it ever complete) and the device stays usable.  While such an init is still
 * pending, a multi-rank group on that device is refused at once (IRIS_E_HIP:
 * start a fresh process; iris_config's abandoned_inits counts them), so failed
 * formations cannot pile up in a long-lived process; 1-rank groups still form.
 * A formed group all-gathers
 * every rank's PCI bus id over its communicators (iris_group_rccl_info).
 * Group calls are blocking and serialised per group, like the device calls.
 *
 * Failure: waiting for an exchange is bounded.  The clock starts when every
 * local device has reached the all-gather (only the peers can hold it up) and
 * RCCL's asynchronous error is polled meanwhile; on expiry or error the
 * group's communicators are aborted (ncclCommAbort), the call returns
 * IRIS_E_HIP, and every later call on the group or its databases fails the
 * same way (the destroys excepted).  A rank whose own enqueue fails aborts too,
 * so its peers see an error rather than a hang.  Bound: IRIS_GROUP_TIMEOUT_MS,
 * iris_group_set_timeout, else max(30 s, 10 x the call's local work). */
#define IRIS_GROUP_ID_BYTES 128
typedef struct iris_group iris_group_t;
typedef struct iris_group_db iris_group_db_t;
typedef struct iris_group_pending iris_group_pending_t;

int iris_group_create(const int *ordinals, uint32_t n, iris_group_t **out);
int iris_group_unique_id(uint8_t id[IRIS_GROUP_ID_BYTES]);
int iris_group_create_rank(int ordinal, uint32_t nranks, uint32_t rank, const uint8_t id[IRIS_GROUP_ID_BYTES],
                           iris_group_t **out);
int iris_group_destroy(iris_group_t *group);
/* ms > 0: the exchange wait bound of this group's later calls; 0: automatic. */
int iris_group_set_timeout(iris_group_t *group, uint32_t ms);
/* local_devices: devices this process drives; ranks: RCCL ranks in the group
 * (all processes); first_rank: the rank of local device 0. */
int iris_group_info(const iris_group_t *group, uint32_t *local_devices, uint32_t *ranks, uint32_t *first_rank);
/* What RCCL itself reports for the group: *comm_ranks = ncclCommCount of its
 * communicators, and (bus_ids may be NULL; len >= ranks * IRIS_GROUP_BUS_ID_BYTES)
 * every rank's device PCI bus id ("0000:05:00.0", NUL-terminated) at
 * bus_ids + rank * IRIS_GROUP_BUS_ID_BYTES, gathered over the group's own RCCL
 * all-gather when it formed. */
#define IRIS_GROUP_BUS_ID_BYTES 32
int iris_group_rccl_info(const iris_group_t *group, uint32_t *comm_ranks, char *bus_ids, size_t len);
/* Local device i of the group (borrowed: valid until iris_group_destroy), e.g.
 * for iris_device_set_profiling / iris_device_kernel_stats. */
int iris_group_device(const iris_group_t *group, uint32_t i, iris_device_t **dev);

/* A sharded database of `total` records of `kind` over the whole group:
 * S = ranks * shards_per_device contiguous shards (shards_per_device >= 1;
 * more than one splits a device's range into several shards, each searched
 * and exchanged separately).  Every record starts empty (a zero mask: never a
 * candidate, as the reference's NaN rows, src/lib.rs:105-106).  layout as
 * iris_db_create_ex.  A process holds the shards of its local devices. */
int iris_group_db_create(iris_group_t *group, int kind, uint64_t total, int layout, uint32_t shards_per_device,
                         iris_group_db_t **out);
int iris_group_db_destroy(iris_group_db_t *gdb);
/* total records; S = shards in the group; the local shards are [first_shard, first_shard + local_shards). */
int iris_group_db_info(const iris_group_db_t *gdb, uint64_t *total, uint32_t *shards, uint32_t *first_shard,
                       uint32_t *local_shards);
/* Local shard i (0 <= i < local_shards): its database (borrowed; searchable with
 * the single-device calls) and the global index of its record 0. */
int iris_group_db_shard(const iris_group_db_t *gdb, uint32_t i, iris_db_t **db, uint64_t *first, uint64_t *count);
/* Fills every local shard with the synthetic records of iris_db_generate
 * (generator index = global index), all local devices in parallel. */
int iris_group_db_generate(iris_group_db_t *gdb, uint64_t seed);
/* records = host records of the global range [index, index+n) (reference
 * layout); the part held by this process's shards is written. */
int iris_group_db_write(iris_group_db_t *gdb, uint64_t index, const void *records, uint64_t n);
/* Reads the global range [index, index+n) back; it must lie in local shards. */
int iris_group_db_read(const iris_group_db_t *gdb, uint64_t index, uint64_t n, void *records);
/* Global record i <- record first+i of a raw record file (iris_db_load_file's
 * formats and DMA path), local shards only, all local devices in parallel; the
 * file must hold first + total records (IRIS_E_RANGE otherwise). */
int iris_group_db_load_file(iris_group_db_t *gdb, const char *path, uint64_t first);

/* 1 query against the whole sharded template database: on every device the
 * query's engine is built, each local shard searched, the winners all-gathered
 * over RCCL and merged; *out = the global (min distance, lowest index) as
 * iris_template_search over the concatenated database (index = global). */
int iris_group_template_search(iris_group_db_t *gdb, const iris_template_t *query, iris_match_t *out);
/* Pipelined form: enqueues the search, the exchange and the merge, returns at
 * once; wait blocks for THAT search and frees the handle (every local device
 * must agree on the merged winner, IRIS_E_HIP otherwise). */
int iris_group_template_search_async(iris_group_db_t *gdb, const iris_template_t *query, iris_group_pending_t **out);
int iris_group_pending_wait(iris_group_pending_t *pending, iris_match_t *out);
/* nq queries in one pass per shard (iris_template_batch_search rules: TILES
 * layout for nq > 3); out[q] = query q's global winner. */
int iris_group_template_batch_search(iris_group_db_t *gdb, const iris_template_t *queries, uint32_t nq,
                                     iris_match_t *out);

#ifdef __cplusplus
}
#endif
#endif /* IRIS_HIP_H */
