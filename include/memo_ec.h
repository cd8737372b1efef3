/*
 * memo_ec.h -- C ABI of the MI355X (gfx950) block erasure codec.
 *
 * Drop-in point in infinit/memo (reference, read-only):
 *   The codec replaces the byte movement of the immutable-block redundancy
 *   path, which in the reference is N-way replication:
 *     store  : Paxos::_store immutable branch + Details::send_immutable_block
 *              src/memo/model/doughnut/consensus/Paxos.cc:1713-1732, 1815-1817,
 *              315-391 (same B bytes sent to `factor` owners)
 *              -> memo_ec_encode_batch (k data + m parity shards, one per owner)
 *     fetch  : Paxos::Details::_fetch immutable branch, Paxos.cc:486-519
 *              (first replica that answers) -> any k shards +
 *              memo_ec_rebuild_batch when a data shard is missing
 *     repair : LocalPeer::_disappeared_evict / _rebalance, Paxos.cc:1012-1246
 *              (copy a surviving replica) -> memo_ec_rebuild_batch of the lost
 *              shards, batched over all under-sharded blocks
 *   The plugin surface it sits behind is unchanged:
 *     consensus::Configuration / Consensus virtuals
 *     src/memo/model/doughnut/Consensus.hh:24-174 (see host/ in this repo for
 *     the ErasureConsensus plugin built on this ABI), payload = the
 *     elle::Buffer of Block::data() (src/memo/model/blocks/Block.hh:142,
 *     elle/src/elle/Buffer.hh:34) handed over as plain pointer + size.
 *
 * Convention: GF(2^8), polynomial 0x11D, generator 2;
 * systematic ISA-L "cauchy1" generator: rows 0..k-1 identity, row i >= k,
 * column j = 1 / (i XOR j).  Shard size S = memo_ec_shard_size(B, k) =
 * round_up(ceil(B / k), 64); a block is zero-padded to k*S bytes and data
 * shard j is bytes [j*S, (j+1)*S) of the padded block.
 *
 * Memory layout of a batch (all pointers are caller-owned):
 *   data   : n blocks x k shards x S bytes, contiguous (block b at b*k*S)
 *   parity : n blocks x m shards x S bytes (parity i of block b at (b*m+i)*S)
 *   rebuild: surv_idx n x k (shard indices in [0,k+m)), surv n x k x S
 *            (the survivors' bytes, in surv_idx order), lost_idx n x e,
 *            out n x e x S (the rebuilt shards, in lost_idx order).
 *
 * Alignment: a shard buffer (data, parity, surv, out, and the same fields of
 * a segment) in MEMO_EC_DEVICE or MEMO_EC_HOST_PINNED memory must be 16-byte
 * aligned, and a verdict array 4-byte aligned in any memory; a call that is
 * handed anything else returns MEMO_EC_EINVAL before anything is enqueued.
 * The kernels reach those buffers as the caller passed them, with 16-byte
 * vector loads and stores and 4-byte atomics on the verdict words; what this
 * part does with such an access at an odd address has not been measured, and
 * shared hardware is no place to find out.  S is a multiple of 64, so every
 * block and shard of an aligned buffer is aligned.  Pageable MEMO_EC_HOST
 * shard buffers may sit at any byte address (the library copies them), as
 * may every index array, the rows of memo_ec_decode_rows and the messages
 * and prefixes of memo_ec_sha256_batch (byte accesses where the address
 * asks for them).  The device-only calls state theirs where they are
 * declared.
 *
 * Threading (mirrors elle::reactor::background, elle/src/elle/reactor/
 * scheduler.cc:562-602, which runs CPU work on <= 16 pool threads): a ctx is
 * used by one thread at a time; distinct ctxs are independent, so each pool
 * thread owns one.  The library owns only device scratch and streams.
 *
 * Errors are returned as negative codes (memo_ec_strerror); the C++ plugin
 * maps them to elle::Error-style exceptions (host/erasure_consensus.hh).
 */
#ifndef MEMO_EC_H
#define MEMO_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEMO_EC_VERSION 2

/* Limits of this implementation. */
#define MEMO_EC_MAX_K 64
#define MEMO_EC_MAX_M 16
#define MEMO_EC_MAX_SEGMENTS 12          /* memo_ec_encode_segments  */
#define MEMO_EC_MAX_REBUILD_SEGMENTS 256 /* memo_ec_rebuild_segments */
/* Shards are shorter than 4 GiB (S < 2^32), and a call's buffers hold less
 * than 2^50 bytes (n * (k + m) * S, n * (k + e) * S; MEMO_EC_ERANGE
 * otherwise, before anything is sized from them). */

typedef struct memo_ec_ctx memo_ec_ctx;

/* Where the buffers of a call live. */
enum memo_ec_where {
    MEMO_EC_HOST = 0,        /* pageable host memory: synchronous call      */
    MEMO_EC_HOST_PINNED = 1, /* page-locked host memory: synchronous call   */
    MEMO_EC_DEVICE = 2       /* device memory of the ctx's GPU: the call is
                                enqueued on the ctx stream and returns; use
                                memo_ec_synchronize for completion/errors   */
};

enum memo_ec_status {
    MEMO_EC_OK = 0,
    MEMO_EC_EINVAL = -1,    /* bad argument (k, m, S, e, pointer, where)    */
    MEMO_EC_ENOMEM = -2,    /* device or pinned allocation failed           */
    MEMO_EC_EHIP = -3,      /* HIP runtime error                            */
    MEMO_EC_ESINGULAR = -4, /* survivor set cannot rebuild (duplicate or
                               out-of-range shard indices)                  */
    MEMO_EC_ENODEV = -5,    /* no such GPU                                  */
    MEMO_EC_ERANGE = -6     /* k or m beyond MEMO_EC_MAX_K / MEMO_EC_MAX_M  */
};

/* One (k, m, S) group of blocks for the fused mixed-geometry encode. */
typedef struct memo_ec_segment {
    int k, m;
    size_t S, n;
    const uint8_t *data; /* device: n x k x S */
    uint8_t *parity;     /* device: n x m x S */
} memo_ec_segment;

/* One (k, m, S) group of blocks of a mixed-geometry rebuild
 * (memo_ec_rebuild_segments).  Per-block patterns (uniform == 0): surv_idx
 * n x k and lost_idx n x e, in the memory `where` names.  One pattern for
 * the group (uniform != 0, the repair of one lost node): surv_idx k and
 * lost_idx e bytes in host memory, as for memo_ec_rebuild_uniform. */
typedef struct memo_ec_rebuild_segment {
    int k, m;
    size_t S, n;
    const uint8_t *surv_idx;
    const uint8_t *surv;     /* n x k x S, in surv_idx order     */
    const uint8_t *lost_idx;
    int e;                   /* lost shards per block, 0..m     */
    int uniform;
    uint8_t *out;            /* n x e x S, in lost_idx order     */
} memo_ec_rebuild_segment;

/* Per-context tuning (memo_ec_ctx_set_option).  Each starts from the
 * environment variable named beside it, read once by memo_ec_ctx_create;
 * a value the option refuses is ignored with a warning on stderr. */
enum memo_ec_option {
    MEMO_EC_OPT_REBUILD_PATH = 1,       /* MEMO_EC_REBUILD_FUSED: -1 auto (default),
                                           0 decode rows + MAC, 1 fused kernel
                                           (the variable: any value > 0 is 1,
                                           any value < 0 is auto)                */
    MEMO_EC_OPT_FUSED_MAX_BYTES = 2,    /* MEMO_EC_FUSED_MAX_MB: auto takes the fused
                                           kernel up to this many survivor bytes
                                           per call (256 MiB)                    */
    MEMO_EC_OPT_ZERO_COPY_BYTES = 3,    /* MEMO_EC_ZC_KB: host calls moving at most
                                           this many bytes run their kernels on
                                           pinned host memory (4 MiB; 0: off)    */
    MEMO_EC_OPT_PIPE_BYTES = 4,         /* MEMO_EC_PIPE_MB: host pipeline batch
                                           (64 MiB)                              */
    MEMO_EC_OPT_COPY_THREADS = 5,       /* MEMO_EC_COPY_THREADS: threads per pageable
                                           bounce copy (0: the shared pool's all;
                                           the variable set to 0 means 1, the
                                           calling thread only)                  */
    MEMO_EC_OPT_MAX_LAUNCH_TILES = 6,   /* MEMO_EC_MAX_LAUNCH_TILES: tiles per MAC
                                           launch (0: the 31-bit grid limit)     */
    MEMO_EC_OPT_XCD_MIN_TILES = 7,      /* MEMO_EC_XCD_MIN_TILES: smallest segment
                                           given the XCD-contiguous tile order   */
    MEMO_EC_OPT_DECODE_WIDE_MAX = 8,    /* MEMO_EC_DECODE_WIDE_MAX: decode-row batches
                                           up to this many blocks take the
                                           column-per-lane kernel (65536)        */
    MEMO_EC_OPT_DECODE_EXACT = 9,       /* MEMO_EC_DECODE_EXACT: exact-k decode
                                           kernels (1)                           */
    MEMO_EC_OPT_DECODE_STAGE = 10,      /* MEMO_EC_DECODE_STAGE: decode rows staged
                                           through LDS (0)                       */
    MEMO_EC_OPT_IMAGE_MIN_TILES = 11,   /* MEMO_EC_IMAGE_MIN_TILES: the decode rows +
                                           MAC rebuild forms per-block product-
                                           table images in HBM for shards of at
                                           least this many whole 4 KiB tiles
                                           (S / 4096) and runs the encode body
                                           over them (1; 0: never, tables built
                                           in LDS)                               */
    MEMO_EC_OPT_IMAGE_MIN_COEFS = 12,   /* MEMO_EC_IMAGE_MIN_COEFS: ... and at least
                                           this many coefficients per block
                                           (padded rows x columns; 40) or a k
                                           without a straight-line MAC body      */
    MEMO_EC_OPT_DECODE_OVERLAP = 13     /* MEMO_EC_DECODE_OVERLAP: a mixed rebuild runs
                                           the decode rows of its later launch
                                           classes on a side stream, overlapping
                                           the earlier MACs (1; 0: all decodes
                                           first, on the call's stream)          */
};

/* Number of GPUs the library can use (0 without a GPU).  A node process
 * spreads its batches over them, one ctx per device per host thread
 * (block-index partition, no collective). */
int memo_ec_device_count(void);

/* Identity of GPU `device`: its PCI bus id ("0000:c1:00.0", pci_len >= 13)
 * and UUID (32 hex digits, uuid_len >= 33), NUL-terminated into the caller's
 * buffers.  A node process that spreads batches over the GPUs records these
 * so a run can prove which physical devices did the work (two ranks naming
 * the same device is a placement error, not a scaling result). */
int memo_ec_device_identity(int device, char *pci_bus_id, size_t pci_len,
                            char *uuid, size_t uuid_len);

/* Context on GPU `device` (its own HIP stream, device scratch). */
int memo_ec_ctx_create(int device, memo_ec_ctx **out);
int memo_ec_ctx_destroy(memo_ec_ctx *ctx);

/* Set / read one memo_ec_option of a ctx (the ctx's owner thread only).
 * MEMO_EC_EINVAL for an unknown option or a value out of its range. */
int memo_ec_ctx_set_option(memo_ec_ctx *ctx, int option, int64_t value);
int memo_ec_ctx_get_option(memo_ec_ctx *ctx, int option, int64_t *value);

/* Enqueue MEMO_EC_DEVICE work on `hip_stream` (a hipStream_t; NULL restores
 * the ctx's own stream).  Lets a caller time kernels with its own events. */
int memo_ec_set_stream(memo_ec_ctx *ctx, void *hip_stream);
void *memo_ec_get_stream(memo_ec_ctx *ctx);

/* Wait for the ctx's enqueued work; returns the first deferred error
 * (e.g. MEMO_EC_ESINGULAR from a device-resident rebuild) and clears it. */
int memo_ec_synchronize(memo_ec_ctx *ctx);

/* round_up(ceil(B / k), 64) */
size_t memo_ec_shard_size(size_t block_bytes, int k);

/* Generator matrix (k+m) x k, row-major, into `out` (host memory). */
int memo_ec_generator(int k, int m, uint8_t *out);

/* parity_i = XOR_j C[k+i][j] * data_j for every block of the batch. */
int memo_ec_encode_batch(memo_ec_ctx *ctx, int k, int m, size_t S, size_t n,
                         const uint8_t *data, uint8_t *parity, int where);

/* Do the k data and m parity shards of each block still agree, and if not,
 * which shard is wrong?  Reads every shard once and writes one word per
 * block:
 * verdict[b] (n words): 0 = the k data and m parity shards of block b agree.
 * Otherwise bits 0..15 (MEMO_EC_VERDICT_MASK) have bit i set iff stored
 * parity shard i differs anywhere from the parity recomputed from the data
 * shards, and bits 16..23 (MEMO_EC_VERDICT_SHARD) name the single shard that
 * explains every mismatch: k + i when parity row i alone differs, the data
 * shard j when all m rows differ and their syndromes s_i (stored XOR
 * recomputed) satisfy s_i[p] * g_0j == g_ij * s_0[p] at every byte p, with
 * g_ij = 1 / ((k + i) ^ j); MEMO_EC_VERDICT_UNLOCATED when no single shard
 * does, and always for m == 1 (one syndrome detects but cannot locate).
 * Bits 24..31 are zero.  A located shard is the code's best explanation, not
 * a proof: with m = 2 two wrong shards can pass for one, so callers check
 * the repaired block against its hash.
 * A mismatch is a result, not an error.  m == 0 or n == 0 writes nothing.
 * `where` as for memo_ec_encode_batch, and names the memory of all three
 * buffers; MEMO_EC_DEVICE: asynchronous on the ctx stream. */
#define MEMO_EC_VERDICT_MASK(v) ((uint32_t)(v) & 0xFFFFu)
#define MEMO_EC_VERDICT_SHARD(v) (((uint32_t)(v) >> 16) & 0xFFu)
#define MEMO_EC_VERDICT_UNLOCATED 0xFFu
int memo_ec_verify_batch(memo_ec_ctx *ctx, int k, int m, size_t S, size_t n,
                         const uint8_t *data, const uint8_t *parity,
                         uint32_t *verdict, int where);

/* Do the k + x shards of each block that a caller has in hand agree, and if
 * not, which one is wrong?  1 <= x <= m; the shards may be any of the k + m,
 * in any order, so a block with a holder down, or a fetch that came back with
 * k + 1 shards, can be judged without its missing shards.
 *
 * have_idx: n x (k + x) shard indices, one byte each, in the memory `where`
 *   names, at any byte address.  Per block, entries 0..k-1 are its basis and
 *   entries k..k+x-1 its spares, in any order.
 * have: n x (k + x) x S bytes, block-major: block b's shard in position t at
 *   have + (b * (k + x) + t) * S.  16-byte aligned in MEMO_EC_DEVICE and
 *   MEMO_EC_HOST_PINNED memory, anywhere in pageable memory.
 * verdict: n words, 4-byte aligned.  With D (x x k) the decode rows of the
 *   spares over the basis and s_r = spare r XOR sum_t D[r][t] * basis_t:
 *   0 = every s_r is zero everywhere.  Otherwise bits 0..15 have bit r set
 *   iff s_r is nonzero somewhere, and bits 16..23 name the shard INDEX (a
 *   value of have_idx) that explains every mismatch: have_idx[b][k + r] when
 *   row r alone differs; have_idx[b][t] when all x rows differ and
 *   s_r[p] * D[0][t] == D[r][t] * s_0[p] at every byte p and row r (at most
 *   one t fits); MEMO_EC_VERDICT_UNLOCATED otherwise, and always for x == 1.
 *   Bits 24..31 are zero.  MEMO_EC_VERDICT_INVALID marks a block whose index
 *   set holds an index >= k + m or a repeat anywhere among its k + x entries;
 *   the other blocks are still judged.  With have_idx = 0..k+m-1 and x = m
 *   the words are those of memo_ec_verify_batch.  As there, a located shard
 *   is the code's best explanation, not a proof.
 * A mismatch and an invalid set are results, not errors: the call returns 0,
 * memo_ec_synchronize reports nothing for them, and an error pending from an
 * earlier call (MEMO_EC_ESINGULAR of a rebuild) is still reported afterwards.
 * MEMO_EC_EINVAL: x < 0 or x > m, S no multiple of 64, a NULL or misaligned
 * pointer, an unknown `where`; MEMO_EC_ERANGE as for the other calls
 * (n * (k + x) * S); all before anything is enqueued.  x == 0 or n == 0
 * writes nothing.  S == 0 is allowed: only the index sets are judged, each
 * word is 0 or MEMO_EC_VERDICT_INVALID, and `have` may be NULL.
 * MEMO_EC_DEVICE: asynchronous on the ctx stream, every word written by the
 * call itself; calls back to back need no synchronize between them.  Host
 * memory goes through the copy pipeline (never zero-copy), in waves cut on
 * block boundaries. */
#define MEMO_EC_VERDICT_INVALID 0xFFFFFFFFu
int memo_ec_check_batch(memo_ec_ctx *ctx, int k, int m, int x, size_t S, size_t n,
                        const uint8_t *have_idx, const uint8_t *have,
                        uint32_t *verdict, int where);

/* memo_ec_check_batch, and the wrong shard of every located block mended in
 * place, on the device, with no host round trip between the two.
 *
 * The call first does exactly what memo_ec_check_batch does, with the same
 * arguments: the same layout of have_idx, have and verdict, the same
 * alignment rules, MEMO_EC_EINVAL / MEMO_EC_ERANGE cases, empty-call rules
 * (x == 0 or n == 0 writes nothing) and meaning of `where`.  `have` is
 * written here, so it is not const.
 *
 * A block is located when its word is nonzero, is not
 * MEMO_EC_VERDICT_INVALID, its shard field is not MEMO_EC_VERDICT_UNLOCATED,
 * and S > 0.  For every located block, the shard in the position q with
 * have_idx[b][q] == MEMO_EC_VERDICT_SHARD(word) is overwritten in `have`.
 * With D (x x k) the block's decode rows of the spares over the basis, the
 * new bytes are, by definition,
 *   q >= k (spare r = q - k):  sum_t D[r][t] * basis_t
 *   q <  k (a basis shard):    inv(D[0][q]) * (spare_0 XOR
 *                                sum_{t != q} D[0][t] * basis_t)
 * -- a one-row multiply-accumulate over k shards that never reads the wrong
 * one.  Bit 24 of the block's word (MEMO_EC_VERDICT_CORRECTED) is then set;
 * bits 0..23 stay the check's word, bits 25..31 are zero.  No other byte of
 * `have` is written: clean, unlocated and invalid blocks are untouched.
 *
 * So a block with one wrong shard gets that shard's true bytes back, and a
 * memo_ec_check_batch of the same buffers afterwards gives 0 for every
 * corrected block.  With x == 1, or S == 0, the call is memo_ec_check_batch.
 * With have_idx = 0..k+m-1 and x = m it corrects what memo_ec_verify_batch
 * locates.  A located shard is the code's best explanation, not a proof:
 * with x = 2 two wrong shards can pass for one, the call then overwrites a
 * shard that may have been right, and the old bytes are not kept.  Callers
 * check the mended block against its hash.
 *
 * A correction is a result, not an error: the return value and
 * memo_ec_synchronize behave as for the check.  MEMO_EC_DEVICE: asynchronous
 * on the ctx stream, no host synchronisation inside the call; calls back to
 * back need no synchronize between them.  Host memory goes through the copy
 * pipeline (never zero-copy), in the check's waves, cut on block boundaries;
 * a wave moves the check's bytes plus S bytes back per corrected block,
 * never the whole wave. */
#define MEMO_EC_VERDICT_CORRECTED(v) ((((uint32_t)(v)) >> 24) & 1u)  /* only for v != MEMO_EC_VERDICT_INVALID */
int memo_ec_correct_batch(memo_ec_ctx *ctx, int k, int m, int x, size_t S, size_t n,
                          const uint8_t *have_idx, uint8_t *have,
                          uint32_t *verdict, int where);

/* memo_ec_check_batch, and for every block it leaves unlocated the TWO wrong
 * shards, when exactly one pair of shards explains every mismatch.
 *
 * The call is memo_ec_check_batch followed by one more kernel over the same
 * buffers: the same arguments, layout of have_idx, have and verdict,
 * alignment rules, MEMO_EC_EINVAL / MEMO_EC_ERANGE cases in the same order
 * before anything is enqueued, empty-call rules (x == 0 or n == 0 writes
 * nothing) and meaning of `where`.  Nothing but verdict words is written.
 *
 * With D (x x k) and the syndromes s_r of the check, let s[p] be the vector
 * (s_0[p], ..., s_{x-1}[p]) at byte p and H = [D | I_x] the x x (k + x)
 * matrix with one column per POSITION q of have_idx: column q < k is D[:, q],
 * column k + r the unit vector e_r.  A set E of positions explains the block
 * when s[p] lies in span{H_q : q in E} at every byte p.  (The check's shard
 * field is "some one position explains".)  The word is memo_ec_check_batch's,
 * bit for bit, unless x >= 3, S > 0, that word is nonzero, is not
 * MEMO_EC_VERDICT_INVALID, its shard field is MEMO_EC_VERDICT_UNLOCATED, and
 * EXACTLY ONE pair of positions {a, b} explains the block.  Then
 *   bits 0..15   stay the check's mask;
 *   bits 16..23  hold the smaller of the two shard INDICES have_idx[b][a],
 *                have_idx[b][b];
 *   bit 24       is zero;
 *   bits 25..31  hold the larger index plus 1 (1..80, as k + m <= 80):
 *                MEMO_EC_VERDICT_HAS_PAIR / MEMO_EC_VERDICT_SHARD2.
 * In every word that names no pair bits 25..31 are zero;
 * MEMO_EC_VERDICT_INVALID stays all ones.
 *
 * The code is MDS, so any min(x, .) columns of H are independent.  x >= 4:
 * at most one pair can explain an unlocated block, so two wrong shards are
 * always named, whatever their bytes.  x == 3: the pair is unique when the
 * syndrome vectors span two dimensions; when they are all proportional (one
 * wrong byte at the same offset of both shards, say) two pairs can explain
 * the block, and the word then stays unlocated.  x <= 2, or S == 0: the call
 * is memo_ec_check_batch.
 *
 * A located pair is the code's best explanation, not a proof: three wrong
 * shards can pass for two (as two can pass for one in the check with x = 2).
 * Callers rebuild the two shards from the others (memo_ec_correct_pair_batch
 * does it on the device) and check the block against its hash.
 * MEMO_EC_VERDICT_SHARD of a pair word gives the smaller index and so reads
 * like a one-shard answer: callers of THIS call test MEMO_EC_VERDICT_HAS_PAIR
 * first.  Only this call and memo_ec_correct_pair_batch produce such words,
 * and memo_ec_correct_batch never sees one.
 *
 * Results are not errors: the return value and memo_ec_synchronize behave as
 * for the check, and the ctx's deferred errors are left alone.
 * MEMO_EC_DEVICE: asynchronous on the ctx stream; calls back to back need no
 * synchronize between them.  Host memory goes through the copy pipeline in
 * the check's waves: the same bytes in, the same words out.  The extra
 * kernel reads the n verdict words, and the shards of the unlocated blocks
 * up to three times more. */
#define MEMO_EC_VERDICT_HAS_PAIR(v) ((uint32_t)(v) != MEMO_EC_VERDICT_INVALID && (((uint32_t)(v)) >> 25) != 0u)
#define MEMO_EC_VERDICT_SHARD2(v) (((((uint32_t)(v)) >> 25) & 0x7Fu) - 1u)  /* the larger index; only if HAS_PAIR */
int memo_ec_check_pair_batch(memo_ec_ctx *ctx, int k, int m, int x, size_t S, size_t n,
                             const uint8_t *have_idx, const uint8_t *have,
                             uint32_t *verdict, int where);

/* memo_ec_check_pair_batch, and every block with one or two wrong shards
 * mended in place, on the device, with no host round trip in between.
 *
 * The arguments, the layout of have_idx, have and verdict, the alignment
 * rules, the MEMO_EC_EINVAL / MEMO_EC_ERANGE cases (same order, before
 * anything is enqueued), the empty-call rules (x == 0 or n == 0 writes
 * nothing) and the meaning of `where` are exactly memo_ec_correct_batch's.
 *
 * Single-located blocks (the check names one shard): the call does what
 * memo_ec_correct_batch does: the same bytes written, the same word (bits
 * 0..23 the check's, bit 24 set, bits 25..31 zero).
 *
 * Pair blocks (memo_ec_check_pair_batch would return a pair word: x >= 3,
 * S > 0, exactly one pair of positions qa < qb explains the block): both named
 * shards are overwritten in `have`, and the word is the pair word with bit 24
 * (MEMO_EC_VERDICT_CORRECTED) set.  MEMO_EC_VERDICT_HAS_PAIR, _SHARD, _SHARD2
 * and _CORRECTED all read correctly from it.
 *
 * Every other block -- clean, invalid, unlocated with no unique pair --: the
 * word is memo_ec_check_pair_batch's, and not a byte of `have` is written.
 *
 * The new bytes of a pair block are, by definition, the rebuild of the two
 * named shards, as memo_ec_rebuild_batch with e = 2 gives it, from the k
 * INPUT POSITIONS of the block taken in this fixed order: basis position j
 * (j < k) is input slot j; the slot of each basis target is filled by a spare
 * position that is not a target, the lowest such spare positions being used
 * in ascending order.  So
 *   two spare targets                  read the k basis shards;
 *   basis target q, spare target k + r read the basis without q, and spare c
 *                                      in slot q: c = 0 if r != 0, else 1;
 *   basis targets q1 < q2              read the basis without them, spare 0 in
 *                                      slot q1 and spare 1 in slot q2.
 * The two targets and the remaining spares are never read.  The code is MDS:
 * any k positions determine the block, so the rebuild is unique; the fixed
 * choice matters only when more than two shards are wrong.
 *
 * So a memo_ec_check_batch of the same buffers afterwards gives 0 for every
 * corrected block, single or pair: a unique explaining pair means that the
 * other k + x - 2 positions lie on one codeword.  As ever this is the code's
 * best explanation, not a proof: three wrong shards can pass for two, the call
 * then overwrites two shards that may have been right, and the old bytes are
 * not kept.  Callers check the mended block against its hash.
 *
 * x <= 2: the call is memo_ec_correct_batch.  S == 0, x == 0 or n == 0: as
 * there.  A correction is a result, not an error: the return value and
 * memo_ec_synchronize behave as for the check, and the ctx's deferred errors
 * are left alone.  MEMO_EC_DEVICE: asynchronous on the ctx stream, no host
 * synchronisation inside the call; calls back to back need no synchronize
 * between them.  Host memory goes through the copy pipeline in the check's
 * waves; a wave moves the check's bytes plus S bytes back per single-corrected
 * block and 2 x S (two copies: the shards need not be adjacent) per
 * pair-corrected block, never the whole wave. */
int memo_ec_correct_pair_batch(memo_ec_ctx *ctx, int k, int m, int x, size_t S, size_t n,
                               const uint8_t *have_idx, uint8_t *have,
                               uint32_t *verdict, int where);

/* Ragged batches: n blocks, each with its own shard size, encoded or verified
 * in one call with no padding byte.
 *
 * sizes[b] = S[b], the shard size of block b: a multiple of 64 below 2^32;
 * 0 is allowed (such a block has no bytes, and its verdict word is 0).  With
 * off[b] = S[0] + ... + S[b-1] and T = off[n]:
 *   data   holds k * T bytes; data shard j of block b is at
 *          data + k * off[b] + j * S[b];
 *   parity holds m * T bytes; parity shard i of block b is at
 *          parity + m * off[b] + i * S[b].
 * Blocks stay block-major with their shards contiguous: with every S[b]
 * equal this is byte for byte the layout of memo_ec_encode_batch.
 *
 * sizes: n entries in HOST memory whatever `where` says (as the patterns of
 * memo_ec_rebuild_uniform are), read only during the call: the caller may
 * free it when the call returns.  Everything about it is checked on the host
 * before anything is enqueued: a size that is no multiple of 64 or is >= 2^32,
 * or a NULL `sizes` with n > 0, returns MEMO_EC_EINVAL; k * T or m * T >= 2^50
 * returns MEMO_EC_ERANGE.  n == 0, T == 0 or m == 0 writes nothing.
 *
 * `where`, pointer alignment (data and parity 16 bytes, verdict 4) and
 * asynchrony are as for memo_ec_encode_batch / memo_ec_verify_batch; the
 * verdict words (n of them) are those of memo_ec_verify_batch.  Ragged calls
 * issued back to back on one ctx need no synchronize between them.  The call
 * stages a block index for its kernels through buffers of the ctx, so it
 * cannot be captured into a HIP graph. */
int memo_ec_encode_ragged(memo_ec_ctx *ctx, int k, int m, size_t n, const size_t *sizes,
                          const uint8_t *data, uint8_t *parity, int where);
int memo_ec_verify_ragged(memo_ec_ctx *ctx, int k, int m, size_t n, const size_t *sizes,
                          const uint8_t *data, const uint8_t *parity,
                          uint32_t *verdict, int where);

/* Rebuild the e lost shards of each block from its k survivors.  A lost
 * index may name a data or a parity shard.  e == 0 is a no-op. */
int memo_ec_rebuild_batch(memo_ec_ctx *ctx, int k, int m, size_t S, size_t n,
                          const uint8_t *surv_idx, const uint8_t *surv,
                          const uint8_t *lost_idx, int e, uint8_t *out,
                          int where);

/* Diagnostic: the memory system's rate for an encode's own traffic.  Runs
 * the tiles, tile order and non-temporal 16-byte loads / stores that
 * memo_ec_encode_batch(k = kin, m = r) runs, with the GF arithmetic
 * replaced by XOR.  mode MEMO_EC_PROBE_COPY: out shard i of block b = XOR
 * of its kin input shards, every byte XOR i; MEMO_EC_PROBE_READ: the loads
 * alone (out unspecified); MEMO_EC_PROBE_WRITE: the stores alone (out
 * unspecified).  Device pointers only (in n x kin x S, out n x r x S), both
 * 16-byte aligned (MEMO_EC_EINVAL otherwise); asynchronous on the ctx stream.  The read and write launches' times
 * added give the "achievable" rate of the codec's roofline: this mix of
 * read and write streams without the cost of interleaving them (bench.py:
 * roofline.achievable, frac_of_achievable). */
enum memo_ec_probe_mode {
    MEMO_EC_PROBE_COPY = 0,
    MEMO_EC_PROBE_READ = 1,
    MEMO_EC_PROBE_WRITE = 2
};
int memo_ec_stream_probe(memo_ec_ctx *ctx, int kin, int r, size_t S, size_t n,
                         const uint8_t *in, uint8_t *out, int mode);

/* Page-locked host memory for MEMO_EC_HOST_PINNED calls (hipHostMalloc):
 * batch buffers the caller reuses, so its host-memory calls skip the
 * library's bounce copies.  NULL on failure.  Free with memo_ec_host_free. */
void *memo_ec_host_alloc(size_t bytes);
int memo_ec_host_free(void *p);

/* Rebuild with ONE erasure pattern for the whole batch: every block lost the
 * shards lost_idx[0..e) and is rebuilt from the survivors surv_idx[0..k)
 * (host pointers: k and e bytes), surv n x k x S in surv_idx order, out
 * n x e x S.  This is the repair of one lost node, where every block that
 * node held shard i of shares a pattern (Paxos::LocalPeer::_disappeared_evict,
 * src/memo/model/doughnut/consensus/Paxos.cc:1012-1087): the decode rows are
 * formed once on the host and their product tables are shared by all
 * blocks, as the encode's parity rows are, so the call runs at encode
 * speed.  An invalid pattern (duplicate or out-of-range index) returns
 * MEMO_EC_ESINGULAR before anything is enqueued.  `where` as for
 * memo_ec_rebuild_batch (surv/out memory only).  The ctx caches the tables
 * of its last 64 patterns; a pattern's first call uploads them
 * synchronously, so make that call before capturing a HIP graph. */
int memo_ec_rebuild_uniform(memo_ec_ctx *ctx, int k, int m, size_t S, size_t n,
                            const uint8_t *surv_idx, const uint8_t *surv,
                            const uint8_t *lost_idx, int e, uint8_t *out,
                            int where);

/* Per-block decode rows (n x e x k bytes, device): row r of block b holds the
 * coefficients of lost_idx[b][r] over the survivors in surv_idx[b] order,
 * i.e. C[lost] * inv(C[surv]) -- computed in closed form (one lane per block,
 * no matrix inversion), as memo_ec_rebuild_batch does before its
 * multiply-accumulate.  Device pointers only, at any byte alignment (rows
 * off a 4-byte boundary are stored byte-wise); asynchronous on the ctx
 * stream; invalid survivor sets give zero rows and MEMO_EC_ESINGULAR at
 * memo_ec_synchronize. */
int memo_ec_decode_rows(memo_ec_ctx *ctx, int k, int m, size_t n,
                        const uint8_t *surv_idx, const uint8_t *lost_idx,
                        int e, uint8_t *rows);

/* Batched encode of up to MEMO_EC_MAX_SEGMENTS device-resident segments
 * with different (k, m, S): segments of one shard-chunk class (same
 * specialised k) share one launch, classes run back to back.  Every
 * segment's data and parity are 16-byte aligned (MEMO_EC_EINVAL otherwise,
 * before anything is enqueued).  Asynchronous on the ctx stream. */
int memo_ec_encode_segments(memo_ec_ctx *ctx, int nseg,
                            const memo_ec_segment *segs);

/* Rebuild of up to MEMO_EC_MAX_REBUILD_SEGMENTS groups with different
 * (k, m, S, e) and per-block or shared erasure patterns in ONE call: the
 * read side of the multi-address fetch, which hands a whole batch of blocks
 * over at once (Consensus::_fetch(vector<AddressVersion>, ReceiveBlock),
 * src/memo/model/doughnut/Consensus.cc:101-124; Paxos::_fetch,
 * src/memo/model/doughnut/consensus/Paxos.cc:1857-1890).  Segments of one
 * shard-chunk class and kind share a launch (per-block patterns: the fused
 * kernel or decode rows + MAC; shared patterns: product tables formed once
 * on the host), classes run back to back.  Every segment is validated, and
 * every shared pattern decoded, before anything is enqueued (a bad shared
 * pattern: MEMO_EC_ESINGULAR).  MEMO_EC_DEVICE: asynchronous on the ctx
 * stream, per-block faults at memo_ec_synchronize; host memory: synchronous
 * through the copy pipeline, per-block faults returned (the other blocks
 * are still rebuilt). */
int memo_ec_rebuild_segments(memo_ec_ctx *ctx, int nseg,
                             const memo_ec_rebuild_segment *segs, int where);

/* Ragged rebuild: n blocks, each with its own shard size, rebuilt in one call
 * with no padding byte.  sizes, off[b] and T are those of
 * memo_ec_encode_ragged (host array, validated before anything is enqueued
 * with the same MEMO_EC_EINVAL / MEMO_EC_ERANGE rules):
 *   surv holds k * T bytes; survivor t of block b, in surv_idx order, is at
 *        surv + k * off[b] + t * S[b];
 *   out  holds e * T bytes; rebuilt shard r, in lost_idx order, is at
 *        out + e * off[b] + r * S[b].
 * With every S[b] equal this is byte for byte the layout, and the output, of
 * memo_ec_rebuild_batch (uniform != 0: memo_ec_rebuild_uniform).
 *
 * One e serves the call, 0 <= e <= m; e == 0, n == 0 or T == 0 writes
 * nothing.
 * uniform == 0: surv_idx is n x k and lost_idx n x e bytes in the memory
 *   `where` names, at any byte alignment.  Every block's pattern is
 *   validated, zero-size blocks included; an invalid one gives a block whose
 *   `out` bytes are all zero while the others are still rebuilt, and
 *   MEMO_EC_ESINGULAR once: at memo_ec_synchronize for MEMO_EC_DEVICE, from
 *   the call itself for host memory.
 * uniform != 0: surv_idx is k and lost_idx e bytes in HOST memory whatever
 *   `where` says; an invalid pattern returns MEMO_EC_ESINGULAR before
 *   anything is enqueued.  Tables come from the ctx's pattern cache, as for
 *   memo_ec_rebuild_uniform.
 *
 * surv and out are 16-byte aligned in MEMO_EC_DEVICE / MEMO_EC_HOST_PINNED
 * memory (MEMO_EC_EINVAL otherwise, before anything is enqueued); pageable
 * buffers may sit at any byte address.  MEMO_EC_DEVICE calls are asynchronous
 * on the ctx stream and need no synchronize between them; host calls up to
 * MEMO_EC_OPT_ZERO_COPY_BYTES run zero-copy, larger ones through the copy
 * pipeline in waves cut on block boundaries.  Per-block patterns always run
 * the decode rows and then the rows multiply-accumulate over ragged tiles
 * (gf_mac_ragged_rows_kernel): MEMO_EC_OPT_REBUILD_PATH and the
 * MEMO_EC_OPT_IMAGE_* options do not apply to this call.  Like the other
 * ragged calls it cannot be captured into a HIP graph. */
int memo_ec_rebuild_ragged(memo_ec_ctx *ctx, int k, int m, size_t n, const size_t *sizes,
                           const uint8_t *surv_idx, const uint8_t *surv,
                           const uint8_t *lost_idx, int e, int uniform,
                           uint8_t *out, int where);

/* Batched SHA-256 (FIPS 180-4): digest_i = SHA-256(prefix_i || msg_i) for
 * i < n, with prefix_i = prefix + i*prefix_stride (prefix_len bytes; 0 for
 * none) and msg_i = msg + i*msg_stride of msg_len[i] bytes (msg_len == NULL:
 * uniform_len for all).  digest: n x 32 bytes.  This is the CHB address hash
 * SHA-256(salt || owner || data) of CHB::_hash_address
 * (src/memo/model/doughnut/CHB.cc:264-289) and of CHB::_validate
 * (CHB.cc:79-99) for a whole batch; the caller sets address byte 31 to the
 * immutable flag (model/Address.hh: flag_byte).  Device pointers only;
 * prefix and msg at any byte alignment, digest 4-byte and msg_len 8-byte
 * aligned (word stores and loads; MEMO_EC_EINVAL otherwise); asynchronous on
 * the ctx stream. */
int memo_ec_sha256_batch(memo_ec_ctx *ctx, size_t n, const uint8_t *prefix,
                         size_t prefix_len, size_t prefix_stride,
                         const uint8_t *msg, size_t msg_stride,
                         const uint64_t *msg_len, size_t uniform_len,
                         uint8_t *digest);

/* Synthetic workload helpers (device memory; asynchronous on the ctx
 * stream).  Bytes and erasure patterns follow DESIGN.md section 6.  The
 * shard buffers (fill's out; gather's data, parity and out) are 16-byte
 * aligned, MEMO_EC_EINVAL otherwise; gather's idx may sit anywhere. */
int memo_ec_fill_blocks(memo_ec_ctx *ctx, uint64_t seed, uint64_t first_block,
                        size_t n, size_t B, int k, size_t S, uint8_t *out);
int memo_ec_erasures(uint64_t seed, uint64_t first_block, size_t n, int k,
                     int m, int e, uint8_t *surv_idx, uint8_t *lost_idx);
/* out[b][r] = shard idx[b][r] of block b, shards drawn from data (index < k)
 * or parity (index >= k).  Device memory; asynchronous. */
int memo_ec_gather_shards(memo_ec_ctx *ctx, int k, int m, size_t S, size_t n,
                          const uint8_t *data, const uint8_t *parity,
                          const uint8_t *idx, int cnt, uint8_t *out);

const char *memo_ec_strerror(int code);
int memo_ec_version(void);
/* SHA-256 (hex) of the sources this library was built from: include/
 * memo_ec.h, memo_amd/csrc/ec_kernels.h, ec_kernels.hip and memo_ec.cpp,
 * concatenated in that order (memo_amd/csrc/Makefile).  Callers compare it
 * with the sources they ship to prove the loaded kernels are theirs. */
const char *memo_ec_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* MEMO_EC_H */
