/*
 * dsx.h -- C ABI of the MI355X-native content-defined chunker (libdsx.so).
 *
 * Drop-in boundary for desync's chunking hot path.  Each entry point names the
 * reference interface it replaces (paths relative to the desync repository):
 *
 *   dsx_params_init      <- NewChunker validation + constants, chunker.go:134-171
 *                           (discriminatorFromAvg chunker.go:13-15, modInverse32
 *                           chunker.go:20-28)
 *   dsx_cut_device       <- the cut list IndexFromFile assembles, make.go:22-163,
 *                           for a blob already resident in HBM
 *   dsx_cut_host         <- IndexFromFile over an in-memory blob (pinned H2D
 *                           pipeline inside the library)
 *   dsx_cut_fd           <- IndexFromFile(ctx, name, ...) on an open file,
 *                           make.go:49-116 (file read + H2D pipelined)
 *   dsx_stream_*         <- Chunker.Next / Advance over an io.Reader,
 *                           chunker.go:206-309 (stdin/pipe path, tar.go:140)
 *   dsx_cancel           <- ctx cancellation -> Interrupted{}, make.go:201-203,
 *                           errors.go:56-58
 *   dsx_shard_*          <- make.go's split-and-align across GPUs: each rank
 *                           chunks its range, then seams are aligned from a
 *                           small all-gathered seam record (syncWith,
 *                           make.go:277-327)
 *   dsx_seed_plan        <- SeedSequencer.Plan, sequencer.go:41-74 (FileSeed /
 *                           nullChunkSeed LongestMatchWith, fileseed.go:42-80,
 *                           nullseed.go:45-74)
 *   dsx_assemble         <- AssembleFile's copy of the plan's segments,
 *                           assemble.go:93-309, for blobs resident in HBM
 *   dsx_store_*          <- a LocalStore with Uncompressed: true (store.go:21-33,
 *                           :98-99, local.go) and ChunkStorage.StoreChunk
 *                           (chunkstorage.go:44-67), for chunks resident in HBM
 *   dsx_chunk_ids_known  <- Digest.Sum (make.go:223) and StoreChunk's HasChunk
 *                           (chunkstorage.go:44-67) for chunks whose bytes the
 *                           store in HBM already holds: compared, not hashed
 *   dsx_store_prune      <- PruneStore.Prune (store.go:35-39, local.go:163-202)
 *                           and RemoveChunk (local.go:69-75), compacting the
 *                           arena in place
 *   dsx_store_copy       <- Copy (copy.go:9-58) between two stores in HBM
 *   dsx_aead_seal/open   <- the AEAD converter of a store with encryption: true
 *                           (encrypt.go:84-101, XChaCha20-Poly1305, the default of
 *                           store.go:149-156), for chunks resident in HBM
 *
 * Conventions (cgo-safe): plain pointers and sizes only; no pointer passed in
 * is retained after a call returns; every function returns 0 or a negative
 * DSX_E_* code; cut lists are chunk END offsets (the caibx table offsets,
 * index.go:106-113), strictly increasing, the last one equal to the length.
 * A context is not thread-safe (like a Chunker, one per goroutine/worker).
 */
#ifndef DSX_H
#define DSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSX_ABI_VERSION 5

/* ---- error codes (negative) ---------------------------------------------- */
enum {
    DSX_OK = 0,
    DSX_E_MIN_TOO_SMALL = -1,    /* "min chunk size too small, must be over 48"   chunker.go:135-137 */
    DSX_E_MIN_GT_MAX = -2,       /* "min chunk size must not be greater than max"  chunker.go:138-140 */
    DSX_E_MIN_GT_AVG = -3,       /* "min chunk size must not be greater than avg"  chunker.go:141-143 */
    DSX_E_AVG_GT_MAX = -4,       /* "avg chunk size must not be greater than max"  chunker.go:144-146 */
    DSX_E_AVG_RANGE = -5,        /* discriminatorFromAvg() <= 0 (Go: panic / implementation-defined) */
    DSX_E_INVAL = -6,            /* bad argument (NULL pointer, bad flags) */
    DSX_E_CAPACITY = -7,         /* output capacity too small; *n_out holds the required count */
    DSX_E_HIP = -8,              /* HIP runtime error (see dsx_last_error) */
    DSX_E_NOMEM = -9,            /* device or pinned allocation failed */
    DSX_E_INTERRUPTED = -10,     /* dsx_cancel() was called: Interrupted{} errors.go:56-58 */
    DSX_E_IO = -11,              /* read() on the file descriptor failed */
    DSX_E_STATE = -12,           /* call not valid in the current stream state */
    DSX_E_INTERNAL = -13,        /* internal consistency check failed */
    DSX_E_RESYNC = -14,          /* dsx_shard_resolve: exchange the seam records again */
    DSX_E_PEER = -15             /* dsx_shard_resolve: another rank's record carries DSX_SEAM_ERROR */
};

/* ---- chunker parameters ----------------------------------------------------
 * Mirrors the Chunker fields of chunker.go:108-131.  Filled by
 * dsx_params_init(); treat as opaque besides min/avg/max/discriminator. */
typedef struct dsx_params {
    uint64_t min, avg, max;
    uint32_t discriminator; /* hDiscriminator */
    uint32_t inverse_odd;   /* hInverseOdd */
    uint32_t qmax;          /* hQMax */
    uint32_t qbias;         /* hQBias */
    int32_t rot;            /* k = trailing zeros of the discriminator (Go stores -k) */
    uint32_t reserved;
} dsx_params_t;

/* NewChunker(r, min, avg, max) validation and constant derivation.
 * Checks run in the order of chunker.go:135-146 and return the matching
 * DSX_E_* code; dsx_strerror() returns the reference's exact message. */
int dsx_params_init(uint64_t min, uint64_t avg, uint64_t max, dsx_params_t *out);
const char *dsx_strerror(int code);
int dsx_abi_version(void);

/* ---- context ---------------------------------------------------------------- */
typedef struct dsx_ctx dsx_ctx_t;

/* Owns HIP streams, device scratch and pinned staging on `device`.
 *
 * One chain state per context.  A *chain call* runs a chunking chain on the
 * context: dsx_cut_device (with DSX_NO_SYNC or without), dsx_cut_device_many,
 * dsx_cut_host, dsx_cut_fd, dsx_index_host, dsx_index_fd, dsx_stream_begin and
 * the stream's batches, dsx_shard_local (and the re-walk or redo inside a
 * resolve).  They all share the context's one chain state and staging list.
 * Every other call is *neutral*: dsx_chunk_ids, dsx_ids_*, the ID sets and
 * dsx_dedup, the seed plans and dsx_assemble*, dsx_store_*, dsx_read_ranges,
 * dsx_chunk_ids_known, dsx_aead_*, dsx_copy, dsx_sync, dsx_get_stats, the
 * stamps.  Neutral calls may run anywhere -- inside a stream, between
 * dsx_shard_local and its resolve, between a queued call and its dsx_result --
 * and change no result.  For the three protocols that span several calls:
 *   - queued calls: any call may run between a DSX_NO_SYNC call and its
 *     dsx_result (dsx_result's synchronous redo is itself a chain call);
 *   - shards: a chain call between dsx_shard_local and the resolve that
 *     returns DSX_OK makes the shard stale: dsx_shard_resolve,
 *     dsx_shard_resolve_async and dsx_shard_collect then return DSX_E_STATE and
 *     write no list, and the caller starts the round over with
 *     dsx_shard_local.  A stale shard never resolves to a list;
 *   - streams: while a stream is unfinished (begun, and not every chunk up to
 *     the end of its input popped, nor ended) a chain call on its context is
 *     refused with DSX_E_STATE before any device work, and the stream goes on
 *     unharmed.  dsx_stream_begin with uncollected queued calls is refused the
 *     same way: collect them with dsx_result first.
 * After such a DSX_E_STATE dsx_last_error names the protocol that was
 * disturbed first ("stream: ...", "queued calls: ...", "shard: ...").  Work
 * that must overlap a stream or a shard round takes a context of its own.
 * An argument refusal (DSX_E_INVAL) comes first and disturbs nothing. */
int dsx_ctx_create(int device, dsx_ctx_t **out);
int dsx_ctx_destroy(dsx_ctx_t *ctx);
/* Human-readable detail for the last DSX_E_HIP / DSX_E_INTERNAL on ctx, and for
 * a DSX_E_STATE of the chain-state rule above
 * (ctx == NULL: the reason the last dsx_ctx_create failed). */
const char *dsx_last_error(dsx_ctx_t *ctx);
/* Request cancellation of the running/next call; it returns DSX_E_INTERRUPTED. */
int dsx_cancel(dsx_ctx_t *ctx);
/* Progress of the running (or last) dsx_index_* / dsx_cut_fd / dsx_cut_host
 * call: *bytes = the end of the last confirmed chunk, relative to the call's
 * `off` -- pb.Set(chunk.Start + chunk.Size) per assembled chunk in
 * IndexFromFile (make.go:134-140).  Monotone within a call, the file length
 * once it succeeded.  Like dsx_cancel, safe to call from another thread while
 * the call runs (it reads pinned memory the device publishes into after each
 * 32 MiB piece's stitch, 32 values per GiB; it never touches the context's
 * streams). */
int dsx_progress(dsx_ctx_t *ctx, uint64_t *bytes);

/* ---- one-shot cut lists ------------------------------------------------------ */
#define DSX_OUT_HOST 0u   /* out_ends is host memory */
#define DSX_OUT_DEVICE 1u /* out_ends is device memory on the ctx's device */
#define DSX_NO_SYNC 2u    /* (device output only) enqueue on the ctx stream and return;
                             up to 8 such calls may be queued (they run in order);
                             dsx_result() waits for the OLDEST and returns its count */
#define DSX_TIMED 16u     /* with DSX_NO_SYNC: record the call's scan/stitch events
                             (dsx_get_stats after its dsx_result reports them); untimed
                             queued calls record none (an event costs ~6 us of stream time) */

/* Device-resident blob (HBM) -> cut list.  d_blob must stay valid until the
 * call (with DSX_NO_SYNC: its dsx_result()) returns -- a queued call that
 * needs the general path (dense candidates, a stitch repair) is re-run from
 * the blob inside dsx_result().  If cap is too small the call returns
 * DSX_E_CAPACITY and *n_out holds the required count (an upper bound of
 * len/min + 2 always suffices; cap == 0 with out_ends == NULL is the counting
 * call).  A failing call writes nothing at or behind out_ends[cap]; a host
 * out_ends is not written at all, what a device out_ends holds below cap is
 * unspecified (a call of several pieces has written the pieces that fitted).
 * The context's next call is not affected.  A queued call's DSX_E_CAPACITY and
 * count come from its dsx_result().  A queued call's stitch publishes its state
 * into pinned host memory and dsx_result() polls it (no event per call).
 * (The diagnostic build libdsx_diag.so also has DSX_FUSE=1: the stitch of a
 * queued one-piece call as tasks inside the next queued calls' scans; the
 * product library does not read it, INTEGRATION.md "Environment".) */
int dsx_cut_device(dsx_ctx_t *ctx, const void *d_blob, uint64_t len, const dsx_params_t *p,
                   uint64_t *out_ends, uint64_t cap, uint64_t *n_out, uint32_t flags);
int dsx_sync(dsx_ctx_t *ctx);
/* Completes the oldest queued DSX_NO_SYNC dsx_cut_device(): waits for it, then
 * returns its status and cut count (its device cut list is valid once this
 * returns DSX_OK).  DSX_E_STATE if no call is queued. */
int dsx_result(dsx_ctx_t *ctx, uint64_t *n_out);

/* ---- many blobs in one call ---------------------------------------------------
 * d_blob[0, len) holds nblobs blobs back to back (the files of a directory, the
 * tensors of a checkpoint, the members of an archive).  blob_ends[nblobs] (host
 * memory) is non-decreasing and its last entry is len; blob i is [B0, B1) =
 * [blob_ends[i-1], blob_ends[i]) with blob_ends[-1] = 0.  Empty blobs are
 * allowed and give no chunk.  One dsx_params_t applies to every blob.
 * The result equals dsx_cut_device(d_blob + B0, B1 - B0) per blob with B0 added
 * to its ends, concatenated in blob order: the chain of chunker.go:206-277
 * restarts at every blob boundary, with B1 in the place of the length.  Every
 * non-empty blob's B1 is in the list and the list is strictly increasing, so it
 * is a valid `ends` argument (start = 0) for dsx_chunk_ids, dsx_store_put and
 * dsx_aead_seal over the same buffer.  Blob i's chunks are
 * out_ends[blob_first[i] .. blob_first[i+1]) and blob_first[nblobs] == *n_out.
 * Small blobs are scanned in groups, one scan launch per group, and their chains
 * are walked side by side; a blob of big_blob bytes or more takes the path of
 * dsx_cut_device on its own.  The options change the cost, never
 * the result.
 * flags: DSX_OUT_HOST or DSX_OUT_DEVICE (where out_ends lives); any other bit,
 * DSX_NO_SYNC included, is DSX_E_INVAL.  The call is synchronous.  If cap is too
 * small it returns DSX_E_CAPACITY with the needed count in *n_out (totals is
 * written, out_ends and blob_first are not); a capacity of len / min + nblobs
 * always suffices.  nblobs == 0 with len == 0: DSX_OK, no chunk.
 * Refused with DSX_E_INVAL before any device work (with a ctx, the reason is in
 * dsx_last_error): a NULL ctx, p or n_out; NULL blob_ends with nblobs > 0; ends
 * that decrease; a last end other than len; nblobs == 0 with len != 0; more than
 * 2^32 - 16 blobs; a NULL d_blob with len > 0; a NULL out_ends with cap > 0;
 * non-zero reserved option fields; group_bytes above 8 GiB.
 * dsx_cancel is honoured between groups (DSX_E_INTERRUPTED).  Queued DSX_NO_SYNC
 * calls of the context are treated as a synchronous dsx_cut_device treats them,
 * and the context's one-blob calls behave as before after this call. */
typedef struct dsx_many_opts {   /* 0 in a field: the library's default */
    uint64_t big_blob;           /* blobs at least this long take the one-blob path (at most 1 GiB is
                                    honoured; default: (4096 - 8) * discriminator, capped likewise) */
    uint64_t group_bytes;        /* at most this many bytes per scan launch (<= 8 GiB, the default) */
    uint64_t reserved[2];        /* must be 0 */
} dsx_many_opts_t;

typedef struct dsx_many_totals {
    uint64_t blobs, empty_blobs, chunks;
    uint64_t groups;             /* scan launches of the batched path */
    uint64_t batched_blobs;      /* cut by the batched walk */
    uint64_t single_blobs;       /* cut by the one-blob path because of big_blob or group_bytes */
    uint64_t redone_blobs;       /* batched first, then re-run on the one-blob path */
    uint64_t reserved;
} dsx_many_totals_t;             /* 64 bytes */

int dsx_cut_device_many(dsx_ctx_t *ctx, const void *d_blob, uint64_t len,
                        const uint64_t *blob_ends, uint64_t nblobs, const dsx_params_t *p,
                        uint64_t *out_ends, uint64_t cap, uint64_t *n_out,
                        uint64_t *blob_first /* host, nblobs + 1, may be NULL */,
                        const dsx_many_opts_t *opts /* may be NULL */,
                        dsx_many_totals_t *totals /* may be NULL */, uint32_t flags);

/* Host-memory blob -> cut list (host).  Pipelined pinned H2D inside. */
int dsx_cut_host(dsx_ctx_t *ctx, const void *h_blob, uint64_t len, const dsx_params_t *p,
                 uint64_t *out_ends, uint64_t cap, uint64_t *n_out);

/* File descriptor range [off, off+len) -> cut list (host).  len == UINT64_MAX
 * means "until EOF".  The fd's file offset is not used or changed (pread). */
int dsx_cut_fd(dsx_ctx_t *ctx, int fd, uint64_t off, uint64_t len, const dsx_params_t *p,
               uint64_t *out_ends, uint64_t cap, uint64_t *n_out);

/* ---- streaming (Chunker.Next / Advance over an io.Reader) -------------------
 * One stream per context (a Chunker owns its context, as each Go Chunker owns
 * its buffer and hash state, chunker.go:108-131).
 * begin:  starts a stream at position 0 with params p (NewChunker).  Returns
 *         DSX_E_STATE while another stream on ctx is unfinished, or while
 *         queued DSX_NO_SYNC calls wait for their dsx_result.  Until the
 *         stream is finished or ended, every other chain call on ctx is
 *         refused ("One chain state per context", at dsx_ctx_create).
 *         (dsx_stream_advance and dsx_stream_flush start a finished stream
 *         again: collect queued calls before them, as before begin.)
 * end:    drops the stream (the context can begin a new one).
 * buffer: room for `want` bytes at the tail of the library's pinned host
 *         buffer; *ptr is where the caller writes them (e.g. the reader
 *         reads straight into it).  Valid until the next call on ctx.
 * commit: the caller wrote n bytes at *ptr.  flags: DSX_STREAM_EOF marks the
 *         end of input; DSX_STREAM_SYNC means no more input is coming for
 *         now (a failed reader): everything held is scanned and collected.
 *         Full 8 MiB batches (128 MiB with chunk IDs) are sent to the GPU
 *         without waiting (H2D + scan + stitch, up to 3 batches in flight).
 * push:   buffer + memcpy + commit (eof != 0: DSX_STREAM_EOF).
 * pop:    start and size of the next confirmed chunk.  Returns 1 if a chunk
 *         was produced, 0 if more input is needed first (or the stream
 *         ended: then dsx_stream_done() is 1), or a negative error.  Blocks
 *         on the GPU only when its result is needed and no input can be
 *         taken first.
 * chunk_data: the bytes of the chunk returned by the last pop or flush (host
 *         memory, valid until the next call on ctx -- Next()'s aliasing
 *         rule, chunker.go:202-205).
 * flush:  Next()'s read-error path (chunker.go:207-211, split(n, err)): all
 *         held bytes after the consumer position as one chunk; chunking then
 *         starts over behind them.
 * advance: Chunker.Advance(n) (chunker.go:292-309): drop n bytes at the
 *         current position (held bytes first, then future input), and
 *         continue as if the stream started there.
 * A chunk is confirmed once the bytes up to its start + max are scanned, as
 * Next() needs len(buf) >= max (chunker.go:207, 221). */
#define DSX_STREAM_EOF 1
#define DSX_STREAM_SYNC 2
int dsx_stream_begin(dsx_ctx_t *ctx, const dsx_params_t *p);
int dsx_stream_end(dsx_ctx_t *ctx);
int dsx_stream_buffer(dsx_ctx_t *ctx, uint64_t want, uint8_t **ptr);
int dsx_stream_commit(dsx_ctx_t *ctx, uint64_t n, int flags);
int dsx_stream_push(dsx_ctx_t *ctx, const void *bytes, uint64_t len, int eof);
int dsx_stream_pop(dsx_ctx_t *ctx, uint64_t *start, uint64_t *size);
int dsx_stream_flush(dsx_ctx_t *ctx, uint64_t *start, uint64_t *size);
int dsx_stream_advance(dsx_ctx_t *ctx, uint64_t n);
int dsx_stream_done(dsx_ctx_t *ctx);
const uint8_t *dsx_stream_chunk_data(dsx_ctx_t *ctx);
/* Chunk IDs next to the cuts (ChunkStream, index.go:138-234: Next() then
 * Digest.Sum of every chunk, index.go:165-169): with algo = DSX_DIGEST_* each
 * batch's chunks are hashed on the GPU right after its stitch, on a side
 * stream that overlaps the next batch.  Only before the first bytes of a
 * chain are scanned (else DSX_E_STATE).  dsx_stream_chunk_id returns the
 * 32-byte ID of the chunk the last pop returned (valid until the next call),
 * or NULL if it has none.  Every popped chunk of a chain with IDs has one, the
 * last chunk of a stream whose bytes a DSX_STREAM_SYNC commit had all scanned
 * before the end of input included; only the chunk of a flush has none. */
int dsx_stream_ids(dsx_ctx_t *ctx, int algo);
/* Up to cap confirmed chunks at once (a binding that hands out Next() results
 * without a call per chunk): the first starts at *start, chunk i ends at
 * ends[i]; with ids non-NULL (dsx_stream_ids on) their 32-byte IDs.  Returns
 * 1 with *n >= 1, or what dsx_stream_pop returns (0: input needed / ended).
 * The chunks' bytes are contiguous from dsx_stream_chunk_data(). */
int dsx_stream_pop_many(dsx_ctx_t *ctx, uint64_t *ends, uint8_t *ids, uint64_t cap,
                        uint64_t *start, uint64_t *n);
/* Gives back the chunks of the last pop_many that end after pos (a binding
 * that consumed only some of them before an Advance or a read error): the
 * consumer position returns to pos (a chunk end of that group) and the
 * chunks after it are queued again. */
int dsx_stream_unpop(dsx_ctx_t *ctx, uint64_t pos);
/* The held stream bytes [*base_pos, *base_pos + *len) at *base (host memory,
 * valid until the next buffer/commit/push/advance/flush/end on ctx). */
int dsx_stream_window(dsx_ctx_t *ctx, const uint8_t **base, uint64_t *base_pos, uint64_t *len);
const uint8_t *dsx_stream_chunk_id(dsx_ctx_t *ctx);
/* The clone of a run of chunks out of the held bytes (index.go:196-200,
 * slices.Clone of each chunk: ChunkStream clones a run at once): a host
 * memcpy of n bytes split over up to `threads` threads of a persistent pool
 * (<= 1: the calling thread alone).  dst and src must not overlap.  No
 * context; no GPU. */
int dsx_host_copy(void *dst, const void *src, uint64_t n, int threads);
/* Digest.Sum (digest.go:22, SHA-512/256) of n host messages ptrs[i] of lens[i]
 * bytes into ids[32 i], on up to `threads` host threads: 8 messages per set of
 * AVX-512 registers, longest first (the scalar form without AVX-512, or with
 * DSX_HOST_SHA_SCALAR in flags).  The same code hashes the long chunks of an
 * index call's last window on the host (DSX_INDEX_HOST_TAIL).
 * No context; no GPU. */
#define DSX_HOST_SHA_SCALAR 1
int dsx_host_sha512_256(const uint8_t *const *ptrs, const uint64_t *lens, uint64_t n, uint8_t *ids,
                        int threads, int flags);

/* ---- multi-GPU shards (split-and-align across ranks) ------------------------
 * A blob of total length `total` is range-sharded; rank r holds
 * [shard_start, shard_start+shard_len) in device memory at d_shard, preceded
 * by `halo` readable bytes (halo >= 48, or halo == 0 only when shard_start==0).
 *
 * dsx_shard_local: chunks the shard speculatively from a virtual cut at
 *   shard_start (make.go's worker at span*i, make.go:94-116) and fills a
 *   fixed-size seam record (dsx_seam_t): the candidates and speculative cuts
 *   of the shard's first 32*max bytes and the chain's exit cut.  The record is
 *   built on the device; `seam` is device memory with DSX_SEAM_DEVICE (then it
 *   can be all-gathered by RCCL in place), host memory otherwise.
 * dsx_shard_resolve: given all ranks' seam records (rank order, host or
 *   device memory per DSX_SEAM_DEVICE), walks the true chain across the seams
 *   (syncWith, make.go:277-298) and writes this rank's final cut list: the
 *   cuts c with shard_start < c <= shard_start+shard_len (host memory, or
 *   device memory with DSX_OUT_DEVICE).
 *   Returns DSX_E_RESYNC when a seam did not converge inside its window (a
 *   zero run across a shard boundary, README.md:114-119): the rank owning
 *   that seam has then re-walked its shard from the true entry cut and
 *   rewritten its record `my_seam` (flag DSX_SEAM_REWALKED); every rank
 *   all-gathers the records again and calls dsx_shard_resolve again (at most
 *   nranks rounds).  The re-walk re-runs only the stitch over the shard's
 *   kept candidate lists (O(candidates), no byte is scanned again).  If the
 *   re-walk itself fails, resolve returns that error and marks `my_seam`
 *   DSX_SEAM_ERROR: the caller all-gathers it once more so that every other
 *   rank's resolve returns DSX_E_PEER instead of waiting for a record that
 *   never comes.  d_shard passed to dsx_shard_local must stay valid until
 *   dsx_shard_resolve returns DSX_OK.  A chain call on ctx between
 *   dsx_shard_local and that resolve makes the shard stale: resolve (and
 *   resolve_async, collect) then return DSX_E_STATE and the round starts over
 *   with dsx_shard_local ("One chain state per context", at dsx_ctx_create).
 *   A resolved shard can be resolved again until the next chain call.
 *   If cap is too small for this rank's list, resolve returns DSX_E_CAPACITY
 *   with the required count in *n_out (shard_len/min + 4 + DSX_SEAM_MAX_CUTS
 *   always suffices) and writes nothing to out_ends, host or device; the
 *   other ranks' results are not affected, and the rank may call resolve
 *   again with a larger cap over the same records.  With DSX_E_RESYNC and
 *   DSX_E_PEER *n_out is 0 and out_ends is not written.
 * Seam records are plain bytes. */
#define DSX_SEAM_MAX_CANDS 1024
#define DSX_SEAM_MAX_CUTS 1024
#define DSX_SEAM_DEVICE 8u      /* flag: seam records are device memory */
#define DSX_SEAM_LAST 1u        /* seam flags: the shard ends the blob */
#define DSX_SEAM_REWALKED 2u    /* seam flags: chain re-walked from the true entry `entry`; the record
                                   carries no window (window_end == shard_start, ncands == ncuts == 0) */
#define DSX_SEAM_ERROR 4u       /* seam flags: the owner failed; every rank's resolve returns DSX_E_PEER */
#define DSX_SEAM_REDO 16u       /* seam flags: an asynchronous dsx_shard_local hit a stitch error; the
                                   owner redoes its shard synchronously (dsx_shard_collect) */
typedef struct dsx_seam {
    uint64_t shard_start, shard_len, total;
    uint64_t first_cand_beyond;   /* the first window candidate that did not fit cands[] (the 1025th
                                     of the shard's first 32*max bytes), or UINT64_MAX */
    uint64_t exit_cut;            /* the shard chain's last cut <= shard end */
    uint64_t window_end;          /* candidates/cuts below cover (shard_start, window_end] */
    uint64_t entry;               /* DSX_SEAM_REWALKED: the entry cut the chain started from */
    uint32_t ncands, ncuts, flags, pad;
    uint64_t cands[DSX_SEAM_MAX_CANDS]; /* candidate positions in (shard_start, window_end] */
    uint64_t cuts[DSX_SEAM_MAX_CUTS];   /* spec chain cuts in (shard_start, window_end] */
} dsx_seam_t;

int dsx_shard_local(dsx_ctx_t *ctx, const void *d_shard, uint64_t halo, uint64_t shard_start,
                    uint64_t shard_len, uint64_t total, const dsx_params_t *p, dsx_seam_t *seam,
                    uint32_t flags);
int dsx_shard_resolve(dsx_ctx_t *ctx, const dsx_seam_t *all, int nranks, int rank,
                      dsx_seam_t *my_seam, uint64_t *out_ends, uint64_t cap, uint64_t *n_out,
                      uint32_t flags);

/* Asynchronous step (device records, device cut list): at most one host wait
 * per converged step.
 *   dsx_shard_local(..., DSX_SEAM_DEVICE | DSX_NO_SYNC) enqueues the scan,
 *     stitch and record on the ctx stream and returns (a stitch error shows up
 *     as DSX_SEAM_REDO in the record instead of a return code);
 *   the caller all-gathers the records on the ctx stream (dsx_ctx_stream);
 *   dsx_shard_resolve_async enqueues the resolve: this rank's final cuts go to
 *     out_ends (device, cap entries) and the round's outcome to the device
 *     int32 *d_code: 0 done, 1 exchange again, 2 failed (a peer's
 *     DSX_SEAM_ERROR, or cap too small);
 *   the caller all-reduces the code words with MAX on the ctx stream (the
 *     ranks' agreement, so a local failure reaches every rank in this round);
 *   dsx_shard_collect waits once, copies the agreed word (d_agreed, device,
 *     or NULL when the caller agrees on the host) to *agreed and returns what
 *     dsx_shard_resolve would: DSX_OK with *n_out, DSX_E_RESYNC (the owner of
 *     a non-converged or DSX_SEAM_REDO seam has re-walked / redone its shard
 *     and rewritten my_seam, device memory), DSX_E_PEER, or an error (then
 *     my_seam is marked DSX_SEAM_ERROR when the failure happened after the
 *     agreement: exchange once more so the peers learn of it).  With an
 *     agreed code of 2 it returns this rank's own failure (DSX_E_CAPACITY,
 *     with the required count in *n_out and nothing written to out_ends) or
 *     DSX_E_PEER (*n_out is 0; a list that fitted has been written).  After
 *     either, the ranks may resolve again over the same records.
 *   dsx_shard_resolve_async needs a non-NULL out_ends even with cap == 0. */
int dsx_shard_resolve_async(dsx_ctx_t *ctx, const dsx_seam_t *all, int nranks, int rank,
                            uint64_t *out_ends, uint64_t cap, int32_t *d_code);
int dsx_shard_collect(dsx_ctx_t *ctx, dsx_seam_t *my_seam, const int32_t *d_agreed,
                      int32_t *agreed, uint64_t *n_out);
/* The ctx's HIP stream (hipStream_t), for ordering a caller's collectives
 * with the library's kernels without host waits.  It is created at the
 * highest stream priority, so it takes an HSA queue of that priority's pool
 * (a caller's streams and RCCL's, at the default priority, do not share it;
 * DESIGN.md 5.1). */
int dsx_ctx_stream(dsx_ctx_t *ctx, void **stream);

/* Synchronous copy of n bytes between any host / device pointers (hipMemcpy
 * with the direction inferred): a binding without its own GPU runtime uses it
 * to move the seam-tail bytes of a shard (the chunk IDs across seams). */
int dsx_copy(dsx_ctx_t *ctx, void *dst, const void *src, uint64_t n);

/* ---- diagnostics ------------------------------------------------------------- */
/* Evaluates the GPU boundary predicate (mode 0: multiply-inverse form of
 * chunker.go:265, mode 1: float-reciprocal form, mode 2: multiply-inverse
 * prefilter + exact re-check (d not a power of two), -1: the one the scan uses)
 * for h in [h0, h0+n) (mod 2^32) against h % d == d-1 and counts mismatches
 * (the check of chunker_test.go:190-213, on the device). */
int dsx_selftest_boundary(dsx_ctx_t *ctx, const dsx_params_t *p, int mode, uint64_t h0,
                          uint64_t n, uint64_t *mismatches);

/* Timeline of the last piece when the context was created with
 * DSX_SCAN_TRACE=1 (libdsx_diag.so only; the product library records none and
 * returns zero records) (s_memrealtime ticks, 100 MHz): *n_scan wave-slot records
 * {start, end, regions} of the line-aligned scan, then *n_walk stitch-walk
 * workgroup records {entry, counts scanned, candidates staged, speculative
 * walks done, staged walks done, s_memtime at staged, s_memtime at
 * speculative walks done, first walk: seek done, first step done, chain
 * done}.  Copies min(cap, 3*n_scan + 10*n_walk) words to out. */
int dsx_debug_trace(dsx_ctx_t *ctx, uint64_t *out, uint64_t cap, uint64_t *n_scan,
                    uint64_t *n_walk);

/* ---- measurement: in-kernel stamps of the scan launches ----------------------
 * (bench.py's roofline; replaces no reference interface.)  Between
 * dsx_stamps_begin and dsx_stamps_end the next max_launches line-scan launches
 * of ctx record, from inside the kernel, the s_memrealtime ticks (100 MHz) of
 * their first wave's first instruction and last wave's last instruction, and
 * the shader-clock cycles (s_memtime) and realtime ticks each wave spent, summed
 * over the waves: duration = (t_last - t_first) / 100 MHz, mean shader clock =
 * wave_cycles / wave_ticks * 100 MHz.  No event or extra kernel runs between
 * the stamped launches.  begin waits for the ctx's queued work; end waits for
 * the stamped launches and copies min(cap, *n) records in launch order. */
typedef struct dsx_scan_stamp {
    uint64_t seq;          /* piece sequence number of the launch */
    uint64_t bytes;        /* bytes the launch scanned (one piece: <= 8 GiB) */
    uint64_t t_first, t_last;
    uint64_t wave_cycles, wave_ticks;
    uint64_t waves;        /* waves of the launch's grid */
    uint64_t reserved;
} dsx_scan_stamp_t;
int dsx_stamps_begin(dsx_ctx_t *ctx, uint64_t max_launches);
int dsx_stamps_end(dsx_ctx_t *ctx, dsx_scan_stamp_t *out, uint64_t cap, uint64_t *n);

/* ---- synthetic inputs (bench / tests; generated on device) ------------------ */
/* bytes [offset, offset+len) of the seeded uniform stream (splitmix64 of the
 * 8-byte word index), written to d_dst. */
int dsx_gen_uniform(dsx_ctx_t *ctx, void *d_dst, uint64_t offset, uint64_t len, uint64_t seed);
/* dedup-realistic stream: 1 MiB blocks; block i is, with probability p_repeat,
 * a copy of a uniformly chosen earlier block j < i, else fresh uniform bytes. */
int dsx_gen_dedup(dsx_ctx_t *ctx, void *d_dst, uint64_t offset, uint64_t len, uint64_t seed,
                  double p_repeat);

/* ---- chunk IDs on the GPU (Digest.Sum per chunk: digest.go:11-29, make.go:223,
 * nullchunk.go:17-23) ------------------------------------------------------- */
#define DSX_DIGEST_SHA512_256 0 /* desync's default Digest (digest.go:22) */
#define DSX_DIGEST_SHA256 1     /* the --digest sha256 alternative (digest.go:28) */
#define DSX_ENDS_DEVICE 4u      /* flag: ends[] is device memory (default: host) */
/* 32-byte IDs of the chunks [start, ends[0]), [ends[0], ends[1]), ... of the
 * device-resident blob d_blob[0..len): ids receives n*32 bytes, host memory
 * by default or device memory with DSX_OUT_DEVICE.  Synchronous.
 * Host ends must not decrease, begin at or above start and end at or below len:
 * DSX_E_INVAL otherwise.  Device ends (DSX_ENDS_DEVICE) are checked per chunk on
 * the device instead:
 *   - a chunk that is not inside the readable bytes -- it starts before them,
 *     reaches beyond len, or its end lies below its start -- gets no ID, and its
 *     32 output bytes are left as they were;
 *   - every other chunk of the call gets its ID, wherever it stands in the list
 *     and on whichever kernel path the call runs.
 * The call answers DSX_OK either way. */
int dsx_chunk_ids(dsx_ctx_t *ctx, const void *d_blob, uint64_t len, uint64_t start,
                  const uint64_t *ends, uint64_t n, void *ids, uint32_t flags, int algo);

/* ---- IndexFromFile on the GPU: cut list + chunk IDs ----------------------------
 * The whole of IndexFromFile's data path (make.go:22-163: chunking, then
 * Digest.Sum of every chunk, make.go:223) for a file descriptor range
 * [off, off+len) or a host-memory blob.  len == UINT64_MAX (fd only) means
 * "to the end", for regular files and block devices alike (GetFileSize,
 * ioctl_linux.go:63-84).  Reader threads pread into pinned staging, the bytes
 * are copied to HBM while the next ones are read, chunked there, and hashed
 * there (algo: DSX_DIGEST_*); files larger than the HBM window
 * (DSX_INDEX_WINDOW, 1 GiB) stream through two alternating windows.  The fd's
 * file offset is not used or changed.
 * out_ends: chunk END offsets relative to off (cap entries); ids: 32 bytes per
 * chunk (cap * 32 bytes); both host memory.  DSX_E_CAPACITY sets *n_out to the
 * required count (len/min + 2 always suffices).  Synchronous; dsx_cancel()
 * interrupts it between 32 MiB pieces (DSX_E_INTERRUPTED).
 * Partial results (IndexFromFile returns the chunks assembled so far with
 * chunkErr or Interrupted{}, make.go:133-162, :201-203): on DSX_E_INTERRUPTED
 * and DSX_E_IO, out_ends / ids hold the confirmed prefix of the chain (every
 * chunk of the pieces stitched before the stop, with its ID) and *n_out its
 * length (0 if no piece was done).  dsx_cut_fd / dsx_cut_host do the same
 * with the cut list alone. */
int dsx_index_fd(dsx_ctx_t *ctx, int fd, uint64_t off, uint64_t len, const dsx_params_t *p,
                 int algo, uint64_t *out_ends, uint8_t *ids, uint64_t cap, uint64_t *n_out);
int dsx_index_host(dsx_ctx_t *ctx, const void *h_blob, uint64_t len, const dsx_params_t *p,
                   int algo, uint64_t *out_ends, uint8_t *ids, uint64_t cap, uint64_t *n_out);

/* ---- chunk IDs of a given chunk list from a file or host memory --------------
 * Digest.Sum of the chunks [start, ends[0]), [ends[0], ends[1]), ... of the
 * bytes [off, off+len) of fd (len == UINT64_MAX: to the end) or of
 * h_blob[0..len): the re-hash of VerifyIndex (verifyindex.go:13-79,
 * fileseed.go:183-196) and of ChopFile's NewChunkWithID check (chop.go:66-80,
 * chunk.go:37-73).  Offsets are relative to off; ends must be non-decreasing
 * with start <= ends[0] and ends[n-1] <= len (else DSX_E_INVAL).  The same
 * pipeline as dsx_index_fd without the scan: only [start, ends[n-1]) is read,
 * through pinned staging into two alternating HBM windows whose overlap is the
 * longest chunk.  ids: n * 32 bytes, host memory.  A file shorter than
 * ends[n-1] gives DSX_E_IO.  Synchronous; dsx_cancel() interrupts it. */
int dsx_ids_fd(dsx_ctx_t *ctx, int fd, uint64_t off, uint64_t len, uint64_t start,
               const uint64_t *ends, uint64_t n, int algo, uint8_t *ids);
int dsx_ids_host(dsx_ctx_t *ctx, const void *h_blob, uint64_t len, uint64_t start,
                 const uint64_t *ends, uint64_t n, int algo, uint8_t *ids);

/* ---- chunk-ID sets on the GPU: dedup, seed lookup, the info report ------------
 * The set questions asked of a chunk list once its IDs exist: which chunks
 * repeat inside the blob (the map of `desync info`, cmd/desync/info.go:135-150,
 * and of the self seed, selfseed.go), which exist in a seed index and where
 * (the `pos` map every FileSeed builds, fileseed.go:24-36: pos[id][0] is the
 * first position), and how many bytes the seed does not cover
 * (info.go:152-170).  The IDs stay in HBM, where dsx_chunk_ids(DSX_OUT_DEVICE)
 * leaves them: a set is a lock-free open-addressing hash table over the
 * 32-byte IDs, built and probed by kernels. */
#define DSX_IDS_DEVICE 32u /* flag: ids[] is device memory (default: host) */
#define DSX_SIZES 64u      /* flag: the ends[] argument holds chunk sizes, not end offsets */

typedef struct dsx_idset dsx_idset_t; /* a set of chunk IDs resident on the ctx's device */
/* Builds a set from n 32-byte IDs (host memory, or device memory with
 * DSX_IDS_DEVICE; duplicates allowed; n == 0 gives an empty set).  The set
 * keeps its own device copy of the IDs: the caller may free ids[] when the
 * call returns.  Seeds from several indexes are concatenated by the caller
 * (info.go:100-114 merges them into one map).  A set belongs to ctx: it is
 * used with that context only, its memory counts in that context's
 * device_bytes, and dsx_ctx_destroy frees the sets still alive.  Synchronous.
 * n > 0xFFFFFFF0 or any other flag bit: DSX_E_INVAL. */
int dsx_idset_create(dsx_ctx_t *ctx, const void *ids, uint64_t n, uint32_t flags,
                     dsx_idset_t **out);
int dsx_idset_destroy(dsx_ctx_t *ctx, dsx_idset_t *set);
/* The number of IDs the set was built from and of distinct IDs among them. */
int dsx_idset_count(const dsx_idset_t *set, uint64_t *n_ids, uint64_t *n_unique);

/* The counters of info.go:135-185 (Total, Unique, InSeed, Size, SizeNotInSeed). */
typedef struct dsx_dedup_totals {
    uint64_t total;            /* n */
    uint64_t unique;           /* first occurrences */
    uint64_t in_seed;          /* first occurrences whose ID is in the seed */
    uint64_t size;             /* ends[n-1]; with DSX_SIZES start + the sum of the sizes */
    uint64_t size_not_in_seed; /* sum of the sizes of first occurrences not in the seed */
} dsx_dedup_totals_t;

/* Dedup of the n chunks [start, ends[0]), [ends[0], ends[1]), ... with the
 * 32-byte IDs ids[] against themselves and, with seed non-NULL, against a
 * seed set of the same context:
 *   first_pos[i] = the lowest j <= i with ids[j] == ids[i]; chunk i is a first
 *                  occurrence exactly when first_pos[i] == i;
 *   seed_pos[i]  = the lowest position of that ID in the seed's ids[], or
 *                  0xFFFFFFFF if the seed does not hold it (FileSeed's
 *                  pos[id][0]); all 0xFFFFFFFF without a seed.
 * Both are exact and the same on every run; either may be NULL.  totals
 * (host memory, may be NULL) counts as info.go does: duplicates are counted
 * once, at their first occurrence.  Chunk i's size is ends[i] - ends[i-1]
 * (ends[0] - start), or ends[i] itself with DSX_SIZES (a hand-built list
 * need not be contiguous).
 * flags: DSX_IDS_DEVICE, DSX_ENDS_DEVICE, DSX_OUT_DEVICE (first_pos and
 * seed_pos are device memory), DSX_SIZES; any other bit is DSX_E_INVAL.
 * n == 0: zero totals, DSX_OK.  n > 0xFFFFFFF0: DSX_E_INVAL.  Host ends that
 * decrease or begin below start: DSX_E_INVAL (dsx_last_error says which).  A
 * seed of another context: DSX_E_INVAL.  Synchronous on the ctx stream; the
 * table and the staged arguments live in the context (device_bytes). */
int dsx_dedup(dsx_ctx_t *ctx, const void *ids, const uint64_t *ends, uint64_t start, uint64_t n,
              const dsx_idset_t *seed, uint32_t *first_pos, uint32_t *seed_pos,
              dsx_dedup_totals_t *totals, uint32_t flags);

/* ---- seed plans and in-HBM assembly: the read side (desync extract) -----------
 * SeedSequencer.Plan (sequencer.go:41-74) walks the target index and takes, at
 * each position, the longest run of consecutive chunks some seed holds
 * (FileSeed.LongestMatchWith fileseed.go:42-80, maxMatchFrom :114-136;
 * nullChunkSeed.LongestMatchWith nullseed.go:45-74); AssembleFile
 * (assemble.go:93-309) copies those runs out of the seed blobs and fills the
 * rest from the store.  Here the plan is a list of plain segments and the
 * assembly one gather kernel over blobs resident in HBM. */
#define DSX_SRC_NULL (-1)   /* segment source: the null seed (zeros) */
#define DSX_SRC_STORE (-2)  /* segment source: the packed store buffer */
#define DSX_STORE_DEVICE 128u /* dsx_assemble flag: the store bytes are device memory */
#define DSX_ASSEMBLE_UNALIGNED 256u /* dsx_assemble flag (measurement, tools/assemble_rate.py): load
                                   each misaligned source word with one unaligned load instead of two
                                   aligned loads and a byte shift; the same bytes are written */
#define DSX_ASSEMBLE_TILE 65536u /* output bytes one workgroup of the gather kernel owns */

/* One plan entry (a SeedSegmentCandidate, sequencer.go:21-25). */
typedef struct dsx_plan_seg {
    uint64_t dst_off;    /* offset of target chunk `first` in the target (start included) */
    uint64_t bytes;      /* the target bytes the segment covers */
    uint64_t src_off;    /* seed: offset of chunk seed_first in the seed blob; store: offset of
                            the chunk in the packed store buffer; null: 0 */
    uint32_t first;      /* target chunks [first, first + count) */
    uint32_t count;
    int32_t source;      /* seed number >= 0, DSX_SRC_NULL or DSX_SRC_STORE */
    uint32_t seed_first; /* position of the first matching chunk in the seed, else 0xFFFFFFFF */
} dsx_plan_seg_t;

typedef struct dsx_plan_totals {
    uint64_t segments;
    uint64_t seed_chunks, seed_bytes;   /* from file seeds */
    uint64_t null_chunks, null_bytes;   /* from the null seed */
    uint64_t store_chunks, store_bytes; /* store segments (one chunk each), repeats included */
    uint64_t store_unique;              /* distinct store chunks: the length of store_chunks[] */
    uint64_t store_len;                 /* length of the packed store buffer */
} dsx_plan_totals_t;

/* One seed of dsx_plan_walk, as 32-bit classes (two IDs are equal exactly when
 * their classes are): tclass[i] is the lowest position in this seed of target
 * chunk i's ID or 0xFFFFFFFF (dsx_dedup's seed_pos), sclass[p] the lowest
 * position in this seed of seed chunk p's ID (the seed's own first_pos),
 * ends[m] the seed's chunk ends (its first chunk starts at 0). */
typedef struct dsx_plan_seed {
    const uint32_t *tclass; /* n words */
    const uint32_t *sclass; /* m words */
    const uint64_t *ends;   /* m words */
    uint64_t m;
} dsx_plan_seed_t;

/* SeedSequencer.Plan over classes.  Host code: no context, no GPU.
 * ends/start/n and first_pos[n] as in dsx_dedup; is_null[n] (may be NULL: no
 * null seed) is one byte per chunk, set where the chunk's ID is the null
 * chunk's; limit caps the chunks of one seed match (0: none; the reference
 * uses 100 when it cannot reflink, fileseed.go:62-68).
 * Per seed, the match at target position cur is the maximum, over every seed
 * position p of class tclass[cur] in ascending order, of the number of
 * consecutive positions matching from (cur, p), replaced only by a strictly
 * greater length (ties go to the lowest p).  Between seeds
 * (SeedSequencer.Next, sequencer.go:56-74): the null seed first
 * (assemble.go:151-158), then the file seeds in the order given; a seed
 * replaces the choice only with strictly more bytes, a file seed's bytes being
 * the seed's own (fileseed.go:156-162) and the null seed's the target's; with
 * no match the segment is one chunk from the store.
 * The packed store buffer holds each distinct store chunk once, in the order
 * of its first occurrence in the target; a repeated store chunk gets the
 * src_off of the first (the effect of selfseed.go without a write-after-write
 * dependency in the output).  store_chunks[] receives the target positions of
 * the distinct store chunks in buffer order: the fetch list.
 * If seg_cap or store_cap is too small: DSX_E_CAPACITY, with totals->segments
 * and totals->store_unique the required counts (the totals are complete).
 * Crafted arrays never index out of bounds; DSX_E_INVAL for an sclass[p] > p
 * or not a fixed point (sclass[sclass[p]] != sclass[p]), a tclass[i] neither
 * < m nor 0xFFFFFFFF or not a fixed point of sclass, first_pos[i] > i, ends
 * that decrease, n or m > 0xFFFFFFF0.
 * Cost: only the positions the sequencer visits are matched.  Runs of one ID
 * are stepped over a run at a time on both sides, and of the positions inside
 * one seed run only the two that can win are tried, so a sparse image (one
 * long run of the null chunk's ID in target and seed) costs work proportional
 * to its runs.  Adversarial periodic inputs (ABAB... in target and seed) have
 * runs of one chunk and stay as expensive as in the reference: every
 * occurrence is tried and every match walked chunk by chunk. */
int dsx_plan_walk(const uint64_t *ends, uint64_t start, uint64_t n, const uint32_t *first_pos,
                  const uint8_t *is_null, const dsx_plan_seed_t *seeds, uint32_t nseeds,
                  uint32_t limit, dsx_plan_seg_t *segs, uint64_t seg_cap, uint32_t *store_chunks,
                  uint64_t store_cap, dsx_plan_totals_t *totals);

/* The plan from IDs: ids/ends/start/n as in dsx_dedup (flags DSX_IDS_DEVICE,
 * DSX_ENDS_DEVICE; any other bit is DSX_E_INVAL); seeds[nseeds] are sets of
 * this context built from each seed index's IDs in order (NewIndexSeed,
 * fileseed.go:24-36), seed_ends[k] the host chunk ends of seed k and
 * seed_counts[k] their number, which must equal the set's dsx_idset_count
 * (else DSX_E_INVAL, as for a seed of another context); null_id is the 32-byte
 * ID of the null chunk (nullseed.go:31) or NULL for no null seed.  The classes
 * are made on the device by the sets' tables (a set keeps its own sclass once
 * built, counted in device_bytes), copied to the host (4 bytes per chunk per
 * seed) and walked by dsx_plan_walk, whose outputs (host memory) and return
 * codes these are.  n == 0: zero segments, DSX_OK.  Synchronous. */
int dsx_seed_plan(dsx_ctx_t *ctx, const void *ids, const uint64_t *ends, uint64_t start,
                  uint64_t n, dsx_idset_t *const *seeds, const uint64_t *const *seed_ends,
                  const uint64_t *seed_counts, uint32_t nseeds, const uint8_t *null_id,
                  uint32_t limit, dsx_plan_seg_t *segs, uint64_t seg_cap, uint32_t *store_chunks,
                  uint64_t store_cap, dsx_plan_totals_t *totals, uint32_t flags);

/* AssembleFile's data path (assemble.go:93-309) for blobs in HBM: gathers the
 * nsegs segments (host memory) into d_out[0..out_len): segment s writes
 * d_out[dst_off, dst_off + bytes) from d_seeds[source] + src_off, from the
 * packed store bytes + src_off (host memory, staged through the context; device
 * memory with DSX_STORE_DEVICE), or as zeros (DSX_SRC_NULL).  Output bytes no
 * segment covers are left untouched.  One kernel, work divided by output bytes
 * (DSX_ASSEMBLE_TILE per workgroup) so one chunk and one 1 GiB run load the
 * device alike.  Synchronous on the ctx stream.
 * Checked on the host before any launch, each DSX_E_INVAL with a
 * dsx_last_error text naming the segment: segments ascending and
 * non-overlapping in dst_off; dst_off + bytes <= out_len; src_off + bytes
 * within the source's length; source < nseeds or one of the two constants;
 * [d_out, d_out + out_len) overlapping no source.  With these the kernel
 * cannot read or write outside the buffers it was given, whatever the plan
 * says.  Flags: DSX_STORE_DEVICE, DSX_ASSEMBLE_UNALIGNED; any other bit:
 * DSX_E_INVAL. */
int dsx_assemble(dsx_ctx_t *ctx, const dsx_plan_seg_t *segs, uint64_t nsegs,
                 const void *const *d_seeds, const uint64_t *seed_lens, uint32_t nseeds,
                 const void *store, uint64_t store_len, void *d_out, uint64_t out_len,
                 uint32_t flags);

/* ---- updating a resident blob in place (assemble.go:29-49, :89-92, extract -k) --
 * The buffer holds an old version (or anything) and becomes the target without
 * a second buffer: chunks that already lie at their place are kept, old bytes
 * that the target holds elsewhere are moved inside the buffer, the rest comes
 * from seeds, the store and zeros.  DESIGN.md 4.6, "In place". */
#define DSX_SRC_SELF (-3)   /* segment source: the buffer's own old content, src_off into it */
#define DSX_SRC_STASH (-4)  /* in a schedule's tables only: the stash, src_off into it */
#define DSX_INPLACE_ASCENDING 2048u  /* flag: visit the windows low to high */
#define DSX_INPLACE_DESCENDING 4096u /* flag: visit them high to low (neither: the smaller stash) */
#define DSX_INPLACE_SAVE 0u  /* launch kind A: buffer -> stash (dst_off is a stash offset) */
#define DSX_INPLACE_WRITE 1u /* launch kind B: stash, buffer, seeds, store, zeros -> buffer */

/* One launch of the gather kernel: the segments out_segs[seg0, seg0 + nsegs),
 * ascending in dst_off, written into the stash (SAVE) or the buffer (WRITE);
 * [lo, hi) spans their destinations.  A WRITE's destinations lie in window
 * `window` of the buffer, a SAVE's SELF sources do. */
typedef struct dsx_inplace_launch {
    uint64_t window;
    uint64_t seg0, nsegs;
    uint64_t lo, hi;
    uint32_t kind;
    uint32_t reserved;
} dsx_inplace_launch_t;

typedef struct dsx_inplace_totals {
    uint64_t windows;       /* windows that issued a launch */
    uint64_t launches;      /* and how many (the needed launch_cap) */
    uint64_t segments;      /* entries of all launch tables (the needed seg_cap) */
    uint64_t kept_chunks, kept_bytes; /* chunks left where they lie */
    uint64_t written_bytes; /* bytes the WRITE launches write */
    uint64_t stash_bytes;   /* bytes that went through the stash */
    uint64_t stash_peak;    /* the most the stash held at once: what stash_cap must allow */
    uint32_t direction;     /* DSX_INPLACE_ASCENDING or DSX_INPLACE_DESCENDING: the one taken */
    uint32_t reserved;
} dsx_inplace_totals_t;

/* The schedule of an in-place assembly.  Host code: no context, no GPU.
 * segs[nsegs]: a plan as dsx_seed_plan returns it, ascending in dst_off, with
 * DSX_SRC_SELF among the sources; ends[n]: the target's chunk ends (the first
 * chunk starts at 0); keep[n] (may be NULL): one byte per chunk, set where the
 * chunk already lies correct at its place; have_len: the old content's length;
 * skew and tile: the gather's tile grid on the buffer (skew = the buffer's
 * address modulo 16, tile = DSX_ASSEMBLE_TILE); window: a positive multiple of
 * tile; flags: at most one of the two direction bits.
 * Dropped: a SELF segment with src_off == dst_off and every chunk whose keep
 * byte is set, whatever the plan chose for it (segments are cut at chunk
 * boundaries by first / count).  Bytes nobody writes are never touched.  The
 * rest is cut into windows of the buffer, byte x in window (x + skew) /
 * window; a window with something to write issues a SAVE launch if old bytes
 * of it are still needed, then a WRITE launch.  A launch never writes what it
 * reads, reads only bytes no earlier launch has written, and a stash range is
 * reused only after the last launch that reads it (dsx_inplace_plan.h has the
 * invariant).  Without a forced direction the one with the smaller stash peak
 * is taken, ascending on a tie.
 * Returns DSX_E_CAPACITY with totals->stash_peak > stash_cap when the stash is
 * too small (nothing is listed), or with totals->launches / ->segments the
 * needed counts when launch_cap / seg_cap are.  Each old byte is saved at most
 * once: stash_peak <= have_len.  Crafted arrays never index out of bounds;
 * DSX_E_INVAL for segments that overlap, descend or exceed new_len, a SELF
 * source beyond have_len, first + count > n, bytes or dst_off that are not
 * those of the chunks named, ends that decrease or exceed new_len, a window
 * that is no positive multiple of tile, skew >= tile, any other flag bit. */
int dsx_inplace_plan(const dsx_plan_seg_t *segs, uint64_t nsegs, const uint64_t *ends, uint64_t n,
                     const uint8_t *keep, uint64_t have_len, uint64_t new_len, uint64_t skew,
                     uint64_t tile, uint64_t window, uint64_t stash_cap, uint32_t flags,
                     dsx_inplace_launch_t *launches, uint64_t launch_cap,
                     dsx_plan_seg_t *out_segs, uint64_t seg_cap, dsx_inplace_totals_t *totals);

/* dsx_assemble into a buffer that holds the old version: d_buf[0, have_len) is
 * the old content, d_buf[0, new_len) becomes the target, both within buf_cap.
 * Runs dsx_inplace_plan with the buffer's skew and DSX_ASSEMBLE_TILE, uploads
 * every launch table at once, takes the stash (stash_peak bytes) from the
 * context's scratch (device_bytes) and enqueues the launches on the ctx stream
 * with no host wait between them; one wait at the end.  window == 0: 128 MiB;
 * stash_cap == 0: 2 x window.  Flags: DSX_STORE_DEVICE, DSX_ASSEMBLE_UNALIGNED
 * and the direction bits.  totals may be NULL.
 * Checked on the host before any launch, each DSX_E_INVAL with a
 * dsx_last_error text naming the segment: dsx_assemble's checks with SELF a
 * known source, dsx_inplace_plan's, new_len <= buf_cap, have_len <= buf_cap,
 * no seed and no device store overlapping [d_buf, d_buf + buf_cap).
 * DSX_E_CAPACITY: the stash is too small, totals->stash_peak says what it
 * takes.  After any refusal the buffer is byte for byte what it was.  Not
 * interruptible (as dsx_store_prune).  If a HIP call fails after the first
 * WRITE launch the error is returned and dsx_last_error says that the buffer
 * holds a partial update.  dsx_assemble itself keeps refusing SELF and an
 * output that overlaps a source. */
int dsx_assemble_inplace(dsx_ctx_t *ctx, const dsx_plan_seg_t *segs, uint64_t nsegs,
                         const uint64_t *ends, uint64_t n, const uint8_t *keep,
                         const void *const *d_seeds, const uint64_t *seed_lens, uint32_t nseeds,
                         const void *store, uint64_t store_len, void *d_buf, uint64_t buf_cap,
                         uint64_t have_len, uint64_t new_len, uint64_t window, uint64_t stash_cap,
                         uint32_t flags, dsx_inplace_totals_t *totals);

/* Which chunks of a target already lie at their place in a buffer of unknown
 * content (assemble.go:38-48): the chunks [0, ends[0]), [ends[0], ends[1]), ...
 * that lie wholly inside d_buf[0, have_len) are hashed where they lie (algo as
 * dsx_chunk_ids) and compared with ids[n * 32]; keep[n] (host memory) receives
 * one byte per chunk, 1 where the ID matches, and *n_kept their number.  A
 * chunk reaching beyond have_len, or (device ends) one whose end lies below its
 * start, is not inside the readable bytes: it is not hashed and not kept, as in
 * dsx_chunk_ids.  That is the normal case here, not malformed input, and such a
 * chunk ends nothing: every other chunk of the call is hashed and compared,
 * wherever it stands in the list and on whichever kernel path the call runs.
 * Only the n bytes come to the host.
 * flags: DSX_IDS_DEVICE, DSX_ENDS_DEVICE; any other bit DSX_E_INVAL.
 * Host ends that decrease: DSX_E_INVAL.  n > 0xFFFFFFF0: DSX_E_INVAL.
 * Synchronous. */
int dsx_chunk_keep(dsx_ctx_t *ctx, const void *d_buf, uint64_t have_len, const uint64_t *ends,
                   uint64_t n, const void *ids, int algo, uint8_t *keep, uint64_t *n_kept,
                   uint32_t flags);

/* ---- a chunk store in HBM: what lies between the write and the read side -------
 * The store desync puts between "which chunks are new" and "a plan plus the
 * chunks no seed holds" (store.go:21-33, local.go, chunkstorage.go), for blobs
 * that live in HBM: a deduplicating, tightly packed arena of chunk bytes keyed
 * by chunk ID, filled from a resident blob by kernels, read in place by
 * dsx_assemble and pruned in place by dsx_store_prune.  The counterpart of a
 * LocalStore with Uncompressed: true (store.go:98-99).  DESIGN.md 4.7 has the
 * layout and the launches of a put and of a prune.
 * A store belongs to the context that created it: it is used with that context
 * only (a store of another context: DSX_E_INVAL with a dsx_last_error text),
 * its memory counts in that context's device_bytes, and dsx_ctx_destroy frees
 * the stores still alive.  Its capacity is fixed at creation and the arena is
 * never reallocated, so its address is stable for the store's life (a prune
 * moves chunks inside it); a store grows by dsx_store_copy into a larger one.
 * Out of scope: the compression converter (zstd) and the AES-256-GCM converter -- dsx_aead_seal / dsx_aead_open
 * below are the XChaCha20-Poly1305 one; persistence inside the library
 * (dsx_store_entries, the arena and dsx_aead_seal are what a caller saves and
 * reloads one with: DeviceStore.WriteLocal / ReadLocal do); use from a second
 * context or GPU. */
typedef struct dsx_store dsx_store_t;

/* A store of up to max_chunks chunks (<= 0xFFFFFFF0) and arena_bytes bytes. */
int dsx_store_create(dsx_ctx_t *ctx, uint64_t arena_bytes, uint64_t max_chunks, dsx_store_t **out);
int dsx_store_destroy(dsx_ctx_t *ctx, dsx_store_t *store);

typedef struct dsx_store_counts {
    uint64_t chunks, bytes, max_chunks, arena_bytes;
} dsx_store_counts_t;
int dsx_store_count(const dsx_store_t *store, dsx_store_counts_t *out);

/* ChunkStorage.StoreChunk (chunkstorage.go:44-67) for every chunk of a resident
 * blob. */
typedef struct dsx_store_put_totals {
    uint64_t total;        /* n */
    uint64_t stored;       /* distinct chunks appended by this call */
    uint64_t stored_bytes;
    uint64_t present;      /* first occurrences in this call whose ID the store already held */
    uint64_t repeats;      /* chunks repeating an earlier chunk of this call: total - stored - present */
} dsx_store_put_totals_t;

/* Stores the chunks [start, ends[0]), [ends[0], ends[1]), ... of d_blob[0..len)
 * (device memory; d_blob[0] is position 0 of the offsets) under the IDs ids[]:
 * ids/ends/start/n as in dsx_dedup without DSX_SIZES; flags DSX_IDS_DEVICE,
 * DSX_ENDS_DEVICE, any other bit DSX_E_INVAL.  The IDs are trusted, as
 * StoreChunk trusts chunk.ID(): dsx_chunk_ids before the put, or
 * dsx_store_verify after it, is the check.  A chunk is appended exactly when it
 * is the first occurrence of its ID in this call and the store does not hold
 * that ID; new chunks are appended in the order of their first occurrence,
 * tightly packed, entry e at [ends[e-1], ends[e]) of the arena; zero-length
 * chunks take an entry of size 0.  The arena, the entry order and the totals
 * (host memory, may be NULL) are exact and the same on every run.
 * All or nothing: with chunks + stored > max_chunks or bytes + stored_bytes >
 * arena_bytes the call returns DSX_E_CAPACITY, the totals say what it would
 * have stored, and the store is unchanged.  Checked before any byte is copied,
 * each DSX_E_INVAL with a dsx_last_error text and the store unchanged: the
 * chunk list (start <= ends[0], non-decreasing, ends[n-1] <= len; host ends on
 * the host, device ends by the selecting kernel) and the blob not overlapping
 * the arena.  No kernel reads outside d_blob[0, len) or writes outside the
 * arena.  n == 0: zero totals, DSX_OK.  n > 0xFFFFFFF0: DSX_E_INVAL.
 * Synchronous on the ctx stream: one host wait between selecting and copying,
 * one at the end. */
int dsx_store_put(dsx_ctx_t *ctx, dsx_store_t *store, const void *d_blob, uint64_t len,
                  const void *ids, const uint64_t *ends, uint64_t start, uint64_t n,
                  dsx_store_put_totals_t *totals, uint32_t flags);

/* HasChunk / GetChunk's lookup (store.go:22-23; ChunkMissing) for n IDs:
 * offs[i] = the arena offset of the chunk with ids[i] or UINT64_MAX if the
 * store does not hold it, sizes[i] = its stored size or 0, *n_missing the
 * number of IDs not held; each output may be NULL.  flags: DSX_IDS_DEVICE,
 * DSX_OUT_DEVICE (offs and sizes are device memory). */
int dsx_store_locate(dsx_ctx_t *ctx, const dsx_store_t *store, const void *ids, uint64_t n,
                     uint64_t *offs, uint64_t *sizes, uint64_t *n_missing, uint32_t flags);

/* ---- chunk IDs by comparison: recognise bytes the store already holds ------------
 * dsx_chunk_ids followed by dsx_store_locate in one call -- Digest.Sum
 * (make.go:223) and then HasChunk inside StoreChunk (chunkstorage.go:44-67) --
 * for version N + 1 of a blob whose version N the store holds.  A chunk whose
 * bytes equal a stored entry's bytes has that entry's ID, and store and blob lie
 * in the same HBM: such a chunk is compared, a streaming read, instead of
 * hashed, a serial chain.  Nothing the caller declares is trusted (no dirty
 * ranges); chunks are matched by content, wherever they moved.  DESIGN.md 4.11
 * has the launches.
 * The contract is exact and does not depend on which path produced an ID:
 *   ids[j]       (n * 32 bytes) is what dsx_chunk_ids writes;
 *   known_off[j] (n words, may be NULL) is what dsx_store_locate writes for that
 *                ID: the arena offset, or UINT64_MAX if the store lacks it.
 * It assumes the store's IDs are those of its bytes under `algo`, as
 * dsx_store_put trusts them (dsx_store_verify is the check): algo must be the
 * digest the store was filled with, else recognised chunks carry the store's
 * IDs and hashed chunks the other digest's.
 * Recognition is only an accelerator.  A chunk's fingerprint -- its size, its
 * first and last min(size, 32) bytes and, from 96 bytes on, the 32 bytes at
 * size / 2 - 16 -- selects up to DSX_KNOWN_TRIES entries of the same size and
 * fingerprint; the chunk's bytes are compared with each; the first equal one
 * gives the ID and the offset.  Every other chunk is hashed and then looked up
 * by ID.  No loop over table slots runs longer than DSX_KNOWN_PROBES: an entry
 * or a chunk that hits a bound is hashed as well.
 * d_blob/len/start/ends/n/algo and DSX_ENDS_DEVICE as in dsx_chunk_ids;
 * DSX_OUT_DEVICE: ids and known_off are device memory; any other flag bit is
 * DSX_E_INVAL.  totals (host memory, may be NULL): recognised + hashed ==
 * chunks always.  ids, known_off and every total but untried (and what
 * depends on which of more than DSX_KNOWN_TRIES equal fingerprints were tried)
 * are the same on every run.
 * Refused with DSX_E_INVAL before any device work, with a dsx_last_error text: a
 * NULL ctx (before HIP is touched); a NULL store or ids; host ends that
 * decrease, begin below start or end beyond len; n > 0xFFFFFFF0; an unknown
 * digest.  A store of another context or a broken one: DSX_E_STATE, as
 * dsx_read_ranges answers them.  n == 0: DSX_OK with zero totals.  The blob may
 * overlap the arena: nothing is written to either.  Synchronous on the ctx
 * stream: one host wait between resolving and hashing, one at the end; the
 * scratch (the fingerprint table is rebuilt by every call) counts in
 * device_bytes. */
#define DSX_KNOWN_TILE 65536u  /* pair bytes one workgroup of the compare owns */
#define DSX_KNOWN_TRIES 4u     /* entries compared with one chunk at most */
#define DSX_KNOWN_PROBES 64u   /* table slots an insert or a probe visits at most */

typedef struct dsx_known_totals {
    uint64_t chunks;                     /* n */
    uint64_t recognised, recognised_bytes; /* chunks that got their ID from an equal entry */
    uint64_t hashed, hashed_bytes;       /* chunks the digest kernels hashed */
    uint64_t pairs;                      /* (chunk, entry) pairs compared */
    uint64_t compared_bytes;             /* the sum of their sizes */
    uint64_t fp_false;                   /* pairs whose bytes differed */
    uint64_t untried;                    /* chunks or entries that hit a bound and fell back to hashing */
    uint64_t reserved;                   /* 0 */
} dsx_known_totals_t;                    /* 80 bytes */

int dsx_chunk_ids_known(dsx_ctx_t *ctx, const dsx_store_t *store,
                        const void *d_blob, uint64_t len, uint64_t start,
                        const uint64_t *ends, uint64_t n, int algo,
                        void *ids /* n*32 */, uint64_t *known_off /* n, may be NULL */,
                        dsx_known_totals_t *totals /* may be NULL */, uint32_t flags);

/* The arena for dsx_assemble: store = *d_arena, store_len = *used, with
 * DSX_STORE_DEVICE. */
int dsx_store_arena(const dsx_store_t *store, const void **d_arena, uint64_t *used);

/* The IDs (n * 32 bytes) and cumulative arena ends of entries [first, first + n),
 * in arena order; either may be NULL.  Host memory, or device with
 * DSX_OUT_DEVICE.  first + n beyond the entries: DSX_E_INVAL. */
int dsx_store_entries(dsx_ctx_t *ctx, const dsx_store_t *store, uint64_t first, uint64_t n,
                      void *ids, uint64_t *ends, uint32_t flags);

/* Points a plan's DSX_SRC_STORE segments at the arena.  ids/n are the target's
 * IDs (host memory, or DSX_IDS_DEVICE), segs[nsegs] host memory.  For every
 * segment with source == DSX_SRC_STORE the store is asked for ids[first]: a
 * chunk it does not hold counts in *n_missing, a stored size different from
 * the segment's bytes in *n_wrong_size ("unexpected size for chunk",
 * assemble.go:75-77); *first_bad is the lowest target position with either
 * problem, else 0xFFFFFFFF.  With both counts zero each such segment's src_off
 * becomes the chunk's arena offset; otherwise segs is left untouched.  DSX_OK
 * in both cases (the counts are the answer).  Other segments are never
 * touched.  first + count > n in any segment: DSX_E_INVAL. */
int dsx_store_resolve(dsx_ctx_t *ctx, const dsx_store_t *store, const void *ids, uint64_t n,
                      dsx_plan_seg_t *segs, uint64_t nsegs, uint64_t *n_missing,
                      uint64_t *n_wrong_size, uint32_t *first_bad, uint32_t flags);

/* LocalStore.Verify (local.go:103-161): re-hashes every stored chunk where it
 * lies (algo: DSX_DIGEST_*, the store does not know which digest made its IDs)
 * and compares the result with the stored IDs on the device.  bad[] (host
 * memory) receives the ascending entry numbers of the mismatches, min(cap,
 * *n_bad) of them, *n_bad the full count.  The computed IDs stay in the
 * context's scratch (device_bytes). */
int dsx_store_verify(dsx_ctx_t *ctx, const dsx_store_t *store, int algo, uint32_t *bad,
                     uint64_t cap, uint64_t *n_bad);

/* PruneStore.Prune (store.go:35-39, local.go:163-202; desync prune merges the
 * IDs of the indexes to keep, cmd/desync/prune.go:44-103) and, with
 * DSX_PRUNE_REMOVE, RemoveChunk (local.go:69-75) for a list: what
 * LocalStore.Verify with repair calls for each bad chunk (local.go:103-131). */
#define DSX_PRUNE_REMOVE 512u  /* ids[] names the chunks to drop (RemoveChunk); default: the chunks to keep (Prune) */

typedef struct dsx_store_prune_totals {
    uint64_t entries;                 /* entries before the call */
    uint64_t kept, kept_bytes;
    uint64_t removed, removed_bytes;
    uint64_t moved, moved_bytes;      /* kept entries whose arena offset changed, and their bytes */
    uint64_t unmatched;               /* distinct IDs of ids[] the store did not hold */
} dsx_store_prune_totals_t;           /* 64 bytes */

/* ids[] holds n 32-byte IDs (host memory, or device memory with
 * DSX_IDS_DEVICE; duplicates allowed).  An entry survives exactly when its ID is
 * among them (n == 0 empties the store), or with DSX_PRUNE_REMOVE exactly when
 * it is not (n == 0 changes nothing).  IDs the store does not hold are no
 * error, as in the reference; totals->unmatched counts the distinct ones.
 * Survivors keep their relative order and are renumbered 0 .. kept-1; the arena
 * is tightly packed again, entry e at [ends[e-1], ends[e]), at the same address;
 * arena bytes at and beyond the new `used` are unspecified.  Every store call
 * answers for the compacted store, and the freed chunks and bytes are there for
 * later puts.  Offsets taken before the prune are stale: a plan resolved with
 * dsx_store_resolve, or the answers of dsx_store_locate, must be asked for
 * again before dsx_assemble reads the arena through them.  Bytes in front of
 * the first removed entry are not moved; if nothing is removed, no arena byte,
 * entry or table slot is written.  The arena, the entries and the totals (host
 * memory, may be NULL) are exact and the same on every run.
 * window: the scratch in bytes the compaction may use (counted in device_bytes,
 * grown once and reused), rounded up to a multiple of DSX_ASSEMBLE_TILE and
 * never more than the arena needs; 0: the default, 256 MiB.  The arena is
 * compacted window by window through that scratch, so each moved byte is read
 * twice and written twice.
 * Refused with DSX_E_INVAL and a dsx_last_error text before any device work:
 * a store of another context, ids == NULL with n > 0, n > 0xFFFFFFF0, any flag
 * bit other than DSX_IDS_DEVICE and DSX_PRUNE_REMOVE.
 * Synchronous on the ctx stream: one host wait after the selection (the
 * totals) and one at the end.  dsx_cancel does not interrupt it: a
 * half-compacted arena is not a store.  If a HIP call fails after the first
 * byte has moved, the store is broken: every later call on it but
 * dsx_store_destroy returns DSX_E_STATE. */
int dsx_store_prune(dsx_ctx_t *ctx, dsx_store_t *store, const void *ids, uint64_t n,
                    uint64_t window, dsx_store_prune_totals_t *totals, uint32_t flags);

/* ---- use tracking and eviction: what makes a store of fixed size a cache --------------
 * The reference has no eviction (cache.go grows without bound and leaves the
 * cleanup to desync prune); nothing here changes what it defines.  Everything
 * is opt-in per store: a store that never calls dsx_store_track allocates
 * nothing more, launches nothing more and behaves as above.
 *
 * dsx_store_track allocates one uint64_t stamp per possible entry (max_chunks
 * words, counted in device_bytes, freed with the store), sets the stamp of
 * every entry already there to 0 and starts the store's clock, a host counter,
 * at 0.  A second call changes nothing; tracking cannot be turned off.  A store
 * of another context: DSX_E_INVAL; a broken one: DSX_E_STATE.
 *
 * The use order of a tracked store is total: ascending (stamp, entry number).
 * Among entries with equal stamps the one appended earlier is older.  From
 * dsx_store_track on:
 *   - dsx_store_put and dsx_store_copy into a tracked store take one new clock
 *     value t = ++clock when accepted and stamp with t every entry the call's
 *     IDs name, appended or found present (one more launch over the call's IDs
 *     behind the append).  A refused call (DSX_E_CAPACITY, DSX_E_INVAL, a copy
 *     with missing > 0) and a call with n == 0 stamp nothing and leave the clock.
 *   - a tracked source of a copy that copied something takes its own ++clock on
 *     the entries that were copied (the stamps and the clock are the one thing
 *     a copy changes of src).
 *   - DSX_COPY_ALL from a tracked source into an empty tracked destination
 *     carries the stamps over instead: entry e of dst gets the stamp of entry e
 *     of src, dst's clock becomes src's, and src is not stamped.  A store grown
 *     by such a copy keeps its use order.
 *   - dsx_store_prune carries the survivors' stamps with their IDs and ends.
 *   - The read calls stamp nothing: dsx_store_locate, dsx_store_resolve,
 *     dsx_read_ranges, dsx_chunk_ids_known, dsx_store_verify, dsx_store_entries
 *     and dsx_assemble run exactly as for an untracked store.  What counts as a
 *     use is the caller's decision, said with dsx_store_touch. */
int dsx_store_track(dsx_ctx_t *ctx, dsx_store_t *store);

/* Stamps the entries that hold ids[] (n 32-byte IDs, host memory, or device
 * memory with DSX_IDS_DEVICE; duplicates allowed).  stamp == DSX_STAMP_NOW: the
 * value is ++clock.  Any other stamp is written as given and clock becomes
 * max(clock, stamp): a caller may use its own logical time, such as a training
 * step.  The clock saturates at UINT64_MAX and never wraps: once a caller's
 * stamp has taken it there, every later ++clock, of a put or a copy too,
 * hands out UINT64_MAX again, and those uses are ordered by entry number alone.
 * IDs the store does not hold are no error; *n_missing (may be NULL)
 * counts the positions not held.  n == 0: DSX_OK, the clock does not advance.
 * Any flag bit other than DSX_IDS_DEVICE, n > 0xFFFFFFF0, ids == NULL with
 * n > 0, a store of another context: DSX_E_INVAL; an untracked or a broken
 * store: DSX_E_STATE with a dsx_last_error text.  Synchronous on the ctx
 * stream: one launch, one host wait. */
#define DSX_STAMP_NOW 0ull
int dsx_store_touch(dsx_ctx_t *ctx, dsx_store_t *store, const void *ids, uint64_t n,
                    uint64_t stamp, uint64_t *n_missing, uint32_t flags);

/* The stamps of entries [first, first + n) (host memory, or device memory with
 * DSX_OUT_DEVICE; may be NULL) and the clock (may be NULL), as
 * dsx_store_entries gives IDs and ends.  An untracked store: DSX_E_STATE. */
int dsx_store_stamps(dsx_ctx_t *ctx, const dsx_store_t *store, uint64_t first, uint64_t n,
                     uint64_t *stamps, uint64_t *clock, uint32_t flags);

#define DSX_EVICT_DRY 8192u /* select, fill the totals and evicted_ids; change nothing of the store */

typedef struct dsx_store_evict_totals {
    uint64_t entries;                 /* before the call */
    uint64_t evicted, evicted_bytes;
    uint64_t kept, kept_bytes;
    uint64_t moved, moved_bytes;      /* as dsx_store_prune counts them */
    uint64_t pinned;                  /* entries the pin list protected */
    uint64_t evictable, evictable_bytes; /* unpinned entries and their bytes, before the call */
    uint64_t cutoff;                  /* the largest stamp evicted, 0 if none */
    uint64_t reserved[2];             /* 0 */
} dsx_store_evict_totals_t;          /* 104 bytes */

/* Removes the least recently used entries of a tracked store until there is
 * room for need_bytes bytes and need_chunks chunks, and compacts the arena as
 * dsx_store_prune does.  The contract is exact and the same on every run:
 * let U be the entries whose ID is not among pin_ids[] (n_pin 32-byte IDs,
 * host memory, or device memory with DSX_IDS_DEVICE; duplicates allowed; IDs
 * the store does not hold are ignored), in ascending (stamp, entry number).
 * The call removes the shortest prefix P of U with
 *     arena_bytes - bytes + bytes(P) >= need_bytes   and
 *     max_chunks - chunks + |P| >= need_chunks.
 * Zero-length entries count as chunks only.  If the empty prefix suffices the
 * call changes no arena byte, entry, stamp or table slot and returns DSX_OK;
 * if not even all of U suffices it returns DSX_E_CAPACITY, the store is
 * unchanged and the totals hold entries, pinned, evictable and
 * evictable_bytes (kept and kept_bytes are the store's).
 * evicted_ids (host memory, may be NULL) receives the IDs of the evicted
 * entries in ascending old entry number, min(cap, evicted) of them.
 * Survivors keep their relative order, are renumbered and keep their stamps;
 * the arena is packed at the same address.  Everything dsx_store_prune says of
 * stale offsets, of `window`, of dsx_cancel and of the broken state after a
 * HIP failure past the first write holds here too.
 * DSX_EVICT_DRY: the selection, the totals (moved and moved_bytes included)
 * and evicted_ids of the call without it; the store is not changed.
 * The victims are chosen on the device (Eviction): the stamps
 * and the pin list never cross to the host.
 * Refused before any device work: an untracked store (DSX_E_STATE with a
 * dsx_last_error text), a broken one (DSX_E_STATE), a store of another context,
 * n_pin > 0xFFFFFFF0, pin_ids == NULL with n_pin > 0, any flag bit other than
 * DSX_IDS_DEVICE and DSX_EVICT_DRY (DSX_E_INVAL).
 * Synchronous on the ctx stream: one host wait after the selection (the totals
 * and the capacity decision) and one at the end. */
int dsx_store_evict(dsx_ctx_t *ctx, dsx_store_t *store,
                    uint64_t need_bytes, uint64_t need_chunks,
                    const void *pin_ids, uint64_t n_pin,
                    uint8_t *evicted_ids, uint64_t cap, uint64_t window,
                    dsx_store_evict_totals_t *totals, uint32_t flags);

/* Copy (copy.go:9-58; desync cache, and what a Cache in front of a store does
 * with every chunk it fetches, cache.go:24-45) between two stores of one
 * context, and what growing a store is made of: DSX_COPY_ALL into a new store
 * of another capacity. */
#define DSX_COPY_ALL 1024u  /* ids == NULL, n == 0: every entry of src, in entry order */

typedef struct dsx_store_copy_totals {
    uint64_t total;          /* n (DSX_COPY_ALL: src's entry count) */
    uint64_t copied, copied_bytes; /* distinct chunks appended to dst by this call */
    uint64_t present;        /* first occurrences in this call that dst already held */
    uint64_t repeats;        /* occurrences repeating an earlier ID of this call */
    uint64_t missing;        /* first occurrences neither dst nor src holds */
    uint64_t first_missing;  /* lowest position in ids[] of one, else UINT64_MAX */
    uint64_t reserved;       /* 0 */
} dsx_store_copy_totals_t;   /* 64 bytes */

/* ids[] holds n 32-byte IDs (host memory, or device memory with
 * DSX_IDS_DEVICE; duplicates allowed).  An ID is copied exactly when it is the
 * first occurrence in this call, dst does not hold it and src does.  dst is
 * asked first (copy.go:27-33): an ID dst holds counts as present whether or not
 * src holds it.  New chunks are appended to dst in the order of their first
 * occurrence in ids[], tightly packed, entry e at [ends[e-1], ends[e]);
 * zero-length chunks take an entry of size 0.  The arena, the entry order and
 * the totals are exact and the same on every run; total == copied + present +
 * repeats + missing.
 * All or nothing.  With missing > 0 the call returns DSX_OK, copies nothing and
 * leaves dst untouched: missing and first_missing are the answer, as the counts
 * of dsx_store_resolve are (copied and copied_bytes then count what the call
 * would have copied of the rest).  With chunks + copied > max_chunks or bytes +
 * copied_bytes > arena_bytes it returns DSX_E_CAPACITY, the totals say what it
 * would have copied, and dst is unchanged.  Both are decided after the
 * selecting launch, before any entry, slot or arena byte of dst is written.
 * DSX_COPY_ALL: the IDs are src's own, read where they lie; into an empty dst
 * the result has the same entries, the same ends and the same used arena bytes
 * as src.
 * Refused with DSX_E_INVAL (and, given a ctx, a dsx_last_error text) before any
 * device work: a NULL ctx, dst, src or totals; dst == src; either store
 * belonging to another context; ids == NULL with n > 0 and no DSX_COPY_ALL;
 * DSX_COPY_ALL with ids != NULL or n != 0; n > 0xFFFFFFF0; any flag bit other
 * than DSX_IDS_DEVICE and DSX_COPY_ALL.  A broken store on either side:
 * DSX_E_STATE.  n == 0 without DSX_COPY_ALL: zero counts (first_missing
 * UINT64_MAX), DSX_OK.
 * Synchronous on the ctx stream: one host wait after the selection, one at the
 * end.  src is only read.  No kernel reads outside src's used arena or writes
 * outside dst's arena. */
int dsx_store_copy(dsx_ctx_t *ctx, dsx_store_t *dst, const dsx_store_t *src,
                   const void *ids, uint64_t n, dsx_store_copy_totals_t *totals, uint32_t flags);

/* ---- byte ranges of an indexed blob, read out of a store ---------------------------
 * What NewIndexReadSeeker / IndexPos.Read (readseeker.go), `desync cat -o -l`
 * (cmd/desync/cat.go:95-105) and mount-index do one chunk at a time: the bytes
 * [off, off + len) of the blob an index describes, taken from the chunks that
 * hold them.  Here many ranges are one call, and neither the index, the
 * store's offsets nor a segment list crosses to the host: DESIGN.md 4.10 has
 * the launches.  The read-side counterpart of dsx_cut_device_many. */
typedef struct dsx_range {
    uint64_t off, len;  /* bytes [off, off + len) of the blob, in the coordinates of ends[]
                           (chunk 0 begins at `start`) */
    uint64_t dst_off;   /* ... go to d_out + dst_off */
} dsx_range_t;          /* 24 bytes */

typedef struct dsx_read_totals {
    uint64_t ranges, bytes;  /* nranges, the sum of their lengths */
    uint64_t pieces;         /* (range, chunk) pairs that share at least one byte */
    uint64_t store_bytes, null_bytes; /* bytes of pieces served by the store / as zeros */
    uint64_t missing;        /* pieces whose chunk the store lacks */
    uint64_t wrong_size;     /* pieces whose stored size (null chunk: null_size) differs from the index's */
    uint64_t beyond;         /* ranges with off < start or off + len > ends[n-1] */
    uint32_t first_bad_range; /* lowest range with any of the three, else 0xFFFFFFFF */
    uint32_t first_bad_chunk; /* lowest chunk position among the bad pieces, else 0xFFFFFFFF */
} dsx_read_totals_t;         /* 72 bytes */

typedef struct dsx_read_piece {
    uint64_t chunk_off;  /* first byte of the piece inside its chunk */
    uint64_t dst_off;    /* where it goes in the output */
    uint64_t bytes;      /* > 0 */
    uint32_t range, chunk; /* positions in ranges[] and in the index */
} dsx_read_piece_t;      /* 32 bytes */

/* ids[] holds the index's n 32-byte chunk IDs and ends[] its n cumulative chunk
 * ends (host memory, or device memory with DSX_IDS_DEVICE / DSX_ENDS_DEVICE);
 * chunk i is the blob's bytes [ends[i-1], ends[i]), ends[-1] = start.  ranges[]
 * is host memory.  A range's bytes are written to d_out[dst_off, dst_off + len)
 * (device memory of out_len bytes); bytes of d_out outside these windows are
 * left untouched.
 * Null chunk (readseeker.go:106-107): a chunk whose ID equals null_id is served
 * as zeros without asking the store, whether or not the store holds it, and
 * counts in null_bytes -- provided its size in the index equals null_size;
 * otherwise it is a wrong_size (:123-126).  null_id == NULL: no null chunk.
 * Every other chunk is looked up in the store: an absent one counts in missing
 * (ChunkMissing, :109-112), one whose stored size differs from the index's in
 * wrong_size ("unexpected size for chunk", :123-126).  A range with off < start
 * or off + len > ends[n-1] (n == 0: > start) counts in beyond; clipping a read
 * at the end of the blob (:157-170) is the caller's, who knows the length.
 * All or nothing: with missing, wrong_size and beyond all zero the bytes are
 * written; otherwise no byte of d_out is written.  Both return DSX_OK: the
 * counts are the answer, as with dsx_store_resolve and dsx_store_copy.
 * Ranges may overlap in the blob and repeat; a range of length 0 produces
 * nothing; chunks of size 0 are no pieces and are not looked up.
 * Refused with DSX_E_INVAL and a dsx_last_error text that names the range,
 * before any device work: a NULL ctx (before HIP is touched), store or totals;
 * an unknown flag bit; a missing array; nranges or n > 0xFFFFFFF0; dst_off +
 * len > out_len; a dst_off below the one before it; destination windows that
 * overlap; an output that overlaps the store's arena; host ends that decrease
 * or begin below start; with host ends, more than 0xFFFFFFF0 (range, chunk)
 * pairs (with device ends this is found after the first launch and nothing
 * has been written).  A store of another context or a broken one: DSX_E_STATE.
 * Device ends are trusted to ascend, as elsewhere; a list that does not makes
 * the counts and the bytes meaningless but no kernel reads outside the index,
 * the store or the ranges or writes outside the ranges' windows (DESIGN.md
 * 4.10), and a chunk whose end lies below its start is a wrong_size.
 * Synchronous on the ctx stream; the scratch counts in device_bytes.  Results
 * are exact and the same on every run. */
int dsx_read_ranges(dsx_ctx_t *ctx, const dsx_store_t *store,
                    const void *ids, const uint64_t *ends, uint64_t start, uint64_t n,
                    const uint8_t *null_id, uint64_t null_size,
                    const dsx_range_t *ranges, uint64_t nranges,
                    void *d_out, uint64_t out_len, dsx_read_totals_t *totals, uint32_t flags);

/* The pieces dsx_read_ranges gathers, in order (by range, then by chunk), on the
 * host and without a context (as dsx_plan_walk and dsx_inplace_plan): the same
 * arithmetic the kernels run (dsx_read_geom.h).  ends[] is host memory.
 * *npieces is always set to the number of pieces; with cap too small the first
 * cap are written and the call returns DSX_E_CAPACITY.  DSX_E_INVAL: a missing
 * array or npieces, ends that decrease or begin below start, a range beyond the
 * blob. */
int dsx_read_plan(const uint64_t *ends, uint64_t start, uint64_t n,
                  const dsx_range_t *ranges, uint64_t nranges,
                  dsx_read_piece_t *pieces, uint64_t cap, uint64_t *npieces);

/* ---- the AEAD store converter: seal and open chunks in HBM -------------------------
 * What a store with `encryption: true` writes and reads (encrypt.go:84-101):
 * every chunk sealed on its own with XChaCha20-Poly1305 under one 256-bit key,
 * exactly Go's chacha20poly1305.NewX(key).Seal(out, nonce, in, nil) with empty
 * additional data.  A record is nonce(24) || ciphertext || tag(16).  DESIGN.md
 * 4.8 has the launches.  AES-256-GCM (the reference's alternative) is not built.
 * Both calls are synchronous on the ctx stream; their scratch counts in
 * device_bytes; the key and everything derived from it is cleared from device
 * memory before they return.  Results are exact and the same on every run.
 * Refused with DSX_E_INVAL and a dsx_last_error text before any device work: a
 * NULL context, key or buffer; an algo other than DSX_AEAD_XCHACHA20_POLY1305;
 * an unknown flag bit; n > 0xFFFFFFF0; ends that decrease, begin below start or
 * lie beyond the buffer; a chunk of more than 2^38 - 64 bytes (ChaCha20's 32-bit
 * block counter starts at 1); input and output that overlap.  out_cap too small:
 * DSX_E_CAPACITY. */
#define DSX_AEAD_XCHACHA20_POLY1305 0
#define DSX_AEAD_NONCE 24
#define DSX_AEAD_OVERHEAD 40   /* nonce + tag */
#define DSX_AEAD_TILE 262144u  /* plaintext bytes one workgroup of the main pass owns */

/* Seals the chunks [start, ends[0]), [ends[0], ends[1]), ... of d_src[0..src_len)
 * (given as in dsx_store_put; ends is host memory, or device memory with
 * DSX_ENDS_DEVICE, then copied to the host for the checks).  Record i is
 * d_out[(ends[i-1] - start) + 40 i, (ends[i] - start) + 40 (i + 1)); out_ends[i]
 * (host memory, may be NULL) is its end.  nonces: n * 24 host bytes, or NULL: the
 * library draws them from getrandom(2) and uses none twice within a call (a
 * caller that passes them answers for never repeating one under a key). */
int dsx_aead_seal(dsx_ctx_t *ctx, int algo, const uint8_t key[32], const void *d_src,
                  uint64_t src_len, const uint64_t *ends, uint64_t start, uint64_t n,
                  const uint8_t *nonces, void *d_out, uint64_t out_cap, uint64_t *out_ends,
                  uint32_t flags);
/* Opens the records [start, rec_ends[0]), [rec_ends[0], rec_ends[1]), ... of
 * d_in[0..in_len) (rec_ends is host memory).  Plaintext i has max(0, record size
 * - 40) bytes; the plaintexts are packed from d_out[0] on, out_ends[i] (host
 * memory, may be NULL) their cumulative ends.  A record of fewer than 40 bytes
 * (under 24: the reference's "no nonce prefix found in chunk") or whose tag does
 * not match is bad: bad[] (host memory) receives the ascending numbers of the
 * bad records, min(cap, *n_bad) of them, *n_bad the full count, as
 * dsx_store_verify does, and the plaintext of every bad record is zero-filled
 * before the call returns (Go's Open releases none).  DSX_OK in both cases: the
 * counts are the answer.  flags: none. */
int dsx_aead_open(dsx_ctx_t *ctx, int algo, const uint8_t key[32], const void *d_in,
                  uint64_t in_len, const uint64_t *rec_ends, uint64_t start, uint64_t n,
                  void *d_out, uint64_t out_cap, uint64_t *out_ends, uint32_t *bad, uint64_t cap,
                  uint64_t *n_bad, uint32_t flags);
/* Diagnostic: the Poly1305 tag (host memory) of d_msg[0..len) under the one-time
 * key otk = r || s, by the device functions of the main and finish passes
 * (tiles, powers of r, the combination).  Through the AEAD r and s cannot be
 * chosen; this reaches the edge cases of the arithmetic mod 2^130 - 5. */
int dsx_selftest_poly1305(dsx_ctx_t *ctx, const uint8_t otk[32], const void *d_msg, uint64_t len,
                          uint8_t tag[16]);

/* ---- statistics (ChunkingStats, make.go:329-341 + scan/stitch timings) ------ */
typedef struct dsx_stats {
    uint64_t chunks;            /* ChunksAccepted */
    uint64_t candidates;        /* reserved, always 0 (the scan's candidate counts stay on the device) */
    uint64_t pieces;            /* scan pieces processed */
    uint64_t repaired_segments; /* segments that needed the sequential repair */
    uint64_t dense_fallbacks;   /* pieces processed on the dense-candidate path */
    float scan_ms, stitch_ms;   /* device time of the last synchronous call (HIP events; 0 after dsx_result) */
    uint64_t chunks_discarded;  /* cuts the stitch computed, then replaced by a repair: ChunksProduced
                                   = chunks + chunks_discarded (make.go:329-341 counts the workers'
                                   discarded overlap chunks too) */
    uint64_t device_bytes;      /* HBM the context holds now (its pipeline buffers; filled in by
                                   dsx_get_stats; the caller's blob and cut list are not counted) */
    uint64_t host_tail_chunks;  /* dsx_index_*: chunks of the last window hashed on the host
                                   (DSX_INDEX_HOST_TAIL) while the GPU hashed the others */
} dsx_stats_t;
int dsx_get_stats(dsx_ctx_t *ctx, dsx_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* DSX_H */
