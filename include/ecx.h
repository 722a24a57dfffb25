/*
 * ecx.h -- C ABI of the MI355X GF(256) erasure engine (libecx.so).
 *
 * This is the drop-in boundary for the reference's coding path
 * (krishnarb3/repair-pipelining, rs/ + clay/ + lrc/).  Every entry point
 * names the reference interface it replaces (file:line; file legend in
 * SURVEY.md section 0.1).  A JVM binding (JNI) maps byte[] / ByteBuffer onto
 * these plain pointers; see INTEGRATION.md.
 *
 * Conventions
 *   - Every function returns int: 0 (ECX_OK) or a non-negative result on
 *     success, a negative ECX_E_* code where the Java code throws.
 *     ecx_last_error() gives the thread-local message.
 *   - "Host" (per-call) entry points take caller-owned host buffers (the Java
 *     byte[][] of the reference).  Above the per-call crossover (ecx_tune.h
 *     "host_exec_kib", default 1 MiB per shard / sub-chunk, measured with 1 and
 *     16 caller threads) the bytes are staged to HBM, one fused kernel applies
 *     the composed GF(256) map and the results are copied back; at or below it
 *     the calling thread applies the same map (AVX-512 GFNI / AVX2, host_exec.cpp),
 *     which is faster than a PCIe round trip there.  That is a latency path of a
 *     device-backed library, not a fallback: without a usable HIP device every
 *     such call returns ECX_E_DEVICE, whatever its size.
 *   - "Batch" entry points take DEVICE pointers (HBM-resident stripes) and a
 *     hipStream_t passed as void*; they only enqueue work.  For the many-stream
 *     RS / LRC-encode maps on batches of >= 256 MiB of input, the first calls of a
 *     new layout time the candidate launch shapes with events on that stream (read
 *     later without blocking) and keep the fastest; every shape writes the same bytes
 *     (ecx_tune.h "layout_select").
 *   - Byte order / layout: a shard or sub-chunk is `byte_count` contiguous
 *     bytes.  Clay stripes are plane-major as in the reference
 *     (ClayCodeErasureDecodingStep.java:84-97): input slot z*n + node,
 *     output slot z*|E| + j.
 *   - Thread safety: all entry points may be called concurrently; codec
 *     objects are immutable after creation except for their internal,
 *     lock-protected map cache.
 */
#ifndef ECX_H
#define ECX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status */
enum ecx_status {
    ECX_OK = 0,
    ECX_E_ILLEGAL_ARGUMENT = -1,  /* IllegalArgumentException (sizes, offsets, counts)  */
    ECX_E_NOT_ENOUGH_SHARDS = -2, /* "Not enough shards present"  ReedSolomon.java:211-213 */
    ECX_E_SINGULAR = -3,          /* "Matrix is singular"          Matrix.java:311-313      */
    ECX_E_TOO_MANY_SHARDS = -4,   /* "too many shards - max is 256" ReedSolomon.java:48-50  */
    ECX_E_INDEX = -5,             /* ArrayIndexOutOfBoundsException (e.g. Clay (k+m)%m!=0) */
    ECX_E_NULL = -6,              /* NullPointerException (decodeMissingSingle, bug B3)    */
    ECX_E_NOMEM = -7,             /* host or device allocation failed                      */
    ECX_E_DEVICE = -10            /* no HIP device / HIP runtime error                     */
};

const char *ecx_status_string(int status);
const char *ecx_last_error(void);
int ecx_version(void);

/* ---------------------------------------------------------------- device */
int ecx_device_count(int *count);
int ecx_set_device(int device);     /* per calling thread */
int ecx_synchronize(void *stream);  /* hipStreamSynchronize(stream) */

/* ---------------------------------------------------------------- Galois.java (host planner) */
int ecx_gf_multiply(int a, int b);               /* Galois.multiply  Galois.java:199-209 */
int ecx_gf_divide(int a, int b);                 /* Galois.divide    Galois.java:214-228 */
int ecx_gf_exp(int a, int n);                    /* Galois.exp       Galois.java:239-254 */
int ecx_gf_tables(int16_t *log_table /*256*/, uint8_t *exp_table /*510*/,
                  uint8_t *mul_table /*65536*/); /* Galois.java:59,103,178 */

/* ---------------------------------------------------------------- Matrix.java (host planner) */
int ecx_matrix_times(const uint8_t *a, int a_rows, int a_cols, const uint8_t *b, int b_rows, int b_cols,
                     uint8_t *out);                              /* Matrix.times   Matrix.java:193-210 */
int ecx_matrix_invert(const uint8_t *m, int n, uint8_t *out);   /* Matrix.invert  Matrix.java:273-346 */

/* ---------------------------------------------------------------- CodingLoop.java (host, GPU-executed) */
/* CodingLoop.codeSomeShards (CodingLoop.java:79-85; default implementation
 * InputOutputByteTableCodingLoop.java:12-44): outputs[o][offset..+byte_count) =
 * sum_i matrix_rows[o*input_count + i] * inputs[i][...].  Outputs are overwritten. */
int ecx_code_some_shards(const uint8_t *matrix_rows, const uint8_t *const *inputs, int input_count,
                         uint8_t *const *outputs, int output_count, int offset, int byte_count);
/* CodingLoop.checkSomeShards (CodingLoop.java:110-117): 1 if to_check equals the
 * coded outputs, 0 otherwise.  temp_buffer is accepted for signature parity and unused. */
int ecx_check_some_shards(const uint8_t *matrix_rows, const uint8_t *const *inputs, int input_count,
                          const uint8_t *const *to_check, int check_count, int offset, int byte_count,
                          uint8_t *temp_buffer);
/* InputOutputByteTableCodingLoopSingle.codeSomeShards (…Single.java:4-20):
 * output (=, or ^= when !is_first_time) matrix_rows[output_index*row_length + index] * input. */
int ecx_code_single(const uint8_t *matrix_rows, int row_length, const uint8_t *input, int index,
                    uint8_t *output, int output_index, int offset, int byte_count, int is_first_time);

/* ---------------------------------------------------------------- ReedSolomon.java */
typedef struct ecx_rs ecx_rs;
/* Codec objects: equal codecs (same k, m -- for Clay also virtual nodes and erased list)
 * are one shared, reference-counted object, so per-file / per-repair creates reuse the
 * compiled device plans.  Every create must be paired with one destroy; the last destroy
 * parks the codec in a bounded cache of 64 idle codecs, and one evicted from it frees its
 * device state.  Do not destroy a codec while batch work enqueued with it is in flight. */
int ecx_rs_create(int data_shards, int parity_shards, ecx_rs **out); /* ReedSolomon.create :34-61 */
void ecx_rs_destroy(ecx_rs *rs);
int ecx_rs_matrix(const ecx_rs *rs, uint8_t *out /* total x data */); /* buildMatrix :373-385 */
/* getDataShardCount / getParityShardCount (ReedSolomon.java:63-75); bindings size their
 * argument checks with it (the JNI shim's checkBuffersAndSizes, :338-363). */
int ecx_rs_shape(const ecx_rs *rs, int *data_shards, int *parity_shards);
int ecx_rs_encode_parity(ecx_rs *rs, uint8_t *const *shards, int shard_count, int shard_length, int offset,
                         int byte_count);                            /* encodeParity :94-108 */
int ecx_rs_encode_parity_single(ecx_rs *rs, const uint8_t *shard, uint8_t *output, int input_index,
                                int output_index, int offset, int byte_count); /* :110-118 */
int ecx_rs_is_parity_correct(ecx_rs *rs, uint8_t *const *shards, int shard_count, int shard_length,
                             int first_byte, int byte_count, uint8_t *temp_buffer,
                             int temp_length);                       /* isParityCorrect :129-178 */
int ecx_rs_decode_missing(ecx_rs *rs, uint8_t *const *shards, const uint8_t *shard_present, int shard_count,
                          int shard_length, int offset, int byte_count); /* decodeMissing :189-286 */
/* decodeMissingSingle :288-333.  outputs[j] are caller arrays written in place
 * (assigned when is_first, XOR-accumulated otherwise). */
int ecx_rs_decode_missing_single(ecx_rs *rs, const uint8_t *shard, int shard_index, int index,
                                 const uint8_t *shard_present, uint8_t *const *outputs, int output_count,
                                 int offset, int byte_count, int is_first);

/* ---------------------------------------------------------------- compiled GF maps (device batch) */
/* An ecx_map is one composed GF(256) linear map (a code + erasure pattern),
 * compiled into the kernel's table format and resident on the device.
 * Batch layout: input slot j of stripe s is at in + s*in_stripe_stride + in_slot[j]*in_slot_stride;
 * output row o goes to out + s*out_stripe_stride + out_slot[o]*out_slot_stride. */
typedef struct ecx_map ecx_map;
int ecx_map_create(const uint8_t *matrix /* n_out x n_in */, int n_out, int n_in, const int *in_slot,
                   const int *out_slot, ecx_map **out);
void ecx_map_destroy(ecx_map *map);
int ecx_map_info(const ecx_map *map, int *n_out, int *n_in, int *nnz);
int ecx_map_matrix(const ecx_map *map, uint8_t *matrix /* n_out x n_in */, int *in_slot, int *out_slot);
/* Largest input and output slot index the map reads / writes (-1 = none).  A batch over
 * nstripes stripes of byte_count bytes touches (nstripes-1)*stripe_stride +
 * max_slot*slot_stride + byte_count bytes of each buffer: the extent a binding checks
 * against the caller's buffer (a Java ByteBuffer's capacity) before any device work. */
int ecx_map_slot_extent(const ecx_map *map, int *max_in_slot, int *max_out_slot);
int ecx_map_apply_batch(const ecx_map *map, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                        uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                        int64_t byte_count, void *stream);

/* ReedSolomon.encodeParity (ReedSolomon.java:94-108) over nstripes device-resident
 * stripes, in place: stripe s's shard i is base + s*stripe_stride + i*shard_stride; the
 * parity shards k..n-1 are overwritten for bytes [offset, offset + byte_count). */
int ecx_rs_encode_parity_batch(ecx_rs *rs, uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                               int64_t nstripes, int64_t offset, int64_t byte_count, void *stream);
/* ReedSolomon.isParityCorrect (ReedSolomon.java:129-178; the "Check" half of
 * ReedSolomonBenchmark.java:73-87,126-149) over nstripes device-resident stripes (same layout
 * as ecx_rs_encode_parity_batch), read-only: verdict[s] (a device byte array of nstripes) is
 * set to 1 when every parity shard of stripe s equals the parity of its data over bytes
 * [offset, offset + byte_count), else 0.  Nothing is written to the shards. */
int ecx_rs_is_parity_correct_batch(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                   int64_t nstripes, int64_t offset, int64_t byte_count, uint8_t *verdict,
                                   void *stream);
/* ReedSolomon.decodeMissing (ReedSolomon.java:189-286) over nstripes device-resident
 * stripes, in place (same layout): every shard with shard_present[i] == 0 is rebuilt,
 * data from the first k present shards (ascending index), parity from all data -- the
 * reference's map exactly.  Fewer than k present: ECX_E_NOT_ENOUGH_SHARDS. */
int ecx_rs_decode_missing_batch(ecx_rs *rs, const uint8_t *shard_present, uint8_t *base, int64_t stripe_stride,
                                int64_t shard_stride, int64_t nstripes, int64_t offset, int64_t byte_count,
                                void *stream);

/* A pattern set: erasure patterns of one codec compiled into one device plan, so that one launch
 * decodes a batch whose stripes miss different shards -- the reference's decodeMissing takes
 * shardPresent per call, i.e. per stripe (ReedSolomon.java:189-286).  The set holds a reference
 * on its codec; it must outlive the work enqueued with it; the first batch call with it on a
 * device uploads the plan and must be made outside stream capture. */
typedef struct ecx_rs_pattern_set ecx_rs_pattern_set;
/* decodeMissing's shardPresent (ReedSolomon.java:189-286) for each pattern of the set.
 * patterns: npatterns x n host flags (1 = present), 1 <= npatterns <= 256; duplicates are
 * allowed.  A pattern with fewer than k present: ECX_E_NOT_ENOUGH_SHARDS; one that misses more
 * than 8 shards: ECX_E_ILLEGAL_ARGUMENT (decode such stripes with ecx_rs_decode_missing_batch). */
int ecx_rs_pattern_set_create(ecx_rs *rs, const uint8_t *patterns, int npatterns, ecx_rs_pattern_set **out);
/* Frees the set and its device plans, and drops its codec reference (ReedSolomon.java:189-286
 * keeps no such state: this is the engine's). */
void ecx_rs_pattern_set_destroy(ecx_rs_pattern_set *set);
/* The set's pattern count, its codec's shard count n, and the largest number of shards a
 * pattern misses (the rows decodeMissing rebuilds, ReedSolomon.java:189-286); each may be NULL. */
int ecx_rs_pattern_set_info(const ecx_rs_pattern_set *set, int *npatterns, int *shards, int *max_missing);
/* decodeMissing (ReedSolomon.java:189-286) per stripe, in place, layout of
 * ecx_rs_decode_missing_batch: stripe s is decoded with pattern pattern_of_stripe[s] (a DEVICE
 * byte array of nstripes); an id with no pattern (>= npatterns), or a pattern with nothing
 * missing, leaves the stripe untouched.  Only enqueues. */
int ecx_rs_decode_missing_batch_mixed(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                      uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                      int64_t nstripes, int64_t offset, int64_t byte_count, void *stream);
/* Host helper for the shardPresent flags of many stripes (ReedSolomon.java:189-286): the
 * distinct rows of present[nstripes][shards] in order of first appearance -> patterns (room for
 * cap rows, 1 <= cap <= 256), their count, and ids[nstripes].  Flags compare as zero / non-zero
 * and are written as 0 / 1.  More distinct rows than cap: ECX_E_ILLEGAL_ARGUMENT. */
int ecx_rs_index_patterns(int shards, const uint8_t *present, int64_t nstripes, uint8_t *patterns, int cap,
                          int *npatterns, uint8_t *ids);

/* The engine's layout contract for RS batches in HBM (the reference
 * keeps every shard in its own byte[], ReedSolomonBenchmark.java:198, so the device layout
 * is the caller's choice).  BLOCKED layout of nstripes stripes of n = k + m shards of
 * byte_count bytes, in block_bytes blocks (full = byte_count / block_bytes, tail = the rest):
 *   body  [nstripes][full][n][block_bytes] at base -- a stripe block-major, the way Clay
 *         stores its sub-chunks plane-major (ClayCodeErasureDecodingStep.java:84-97);
 *   tails [nstripes][n][tail] at base + nstripes * full * n * block_bytes.
 * It occupies exactly nstripes * n * byte_count bytes.  Measured against the natural
 * back-to-back shards (scripts/rs_layout_contract.py): RS(17,3) encodeParity on 200,000-B
 * shards 0.695 -> 0.760 of HBM (32 KiB blocks), RS(12,4) 2-erasure decode on 4 MiB shards
 * 0.754 -> 0.816 (64 KiB blocks).
 * ecx_rs_blocked_layout fills layout[3] = {block_bytes, full, tail} for RS(k, m) and a shard
 * size: the largest power of two with n blocks within 1 MiB (4 KiB..1 MiB), or one block of
 * byte_count bytes below that. */
int ecx_rs_blocked_layout(int data_shards, int parity_shards, int64_t byte_count, int64_t *layout);
/* The recommended shard pitch of the plain [stripe][shard][pitch] layout when the caller cannot
 * block: the smallest odd multiple of 4 KiB >= byte_count (RS(12,4) 4 MiB: 0.754 -> 0.789;
 * RS(17,3) 200,000 B: 0.695 -> 0.718). */
int ecx_rs_recommended_pitch(int data_shards, int parity_shards, int64_t byte_count, int64_t *pitch);
/* ecx_rs_encode_parity_batch over the blocked layout (block_bytes > 0; 0 = the recommended
 * block), in place: two launches, the full blocks and the tails, on `stream`. */
int ecx_rs_encode_parity_blocked_batch(ecx_rs *rs, uint8_t *base, int64_t nstripes, int64_t byte_count,
                                       int64_t block_bytes, void *stream);
/* ecx_rs_decode_missing_batch over the blocked layout, in place (the same map). */
int ecx_rs_decode_missing_blocked_batch(ecx_rs *rs, const uint8_t *shard_present, uint8_t *base, int64_t nstripes,
                                        int64_t byte_count, int64_t block_bytes, void *stream);
/* ReedSolomon.isParityCorrect (ReedSolomon.java:129-178) over the blocked layout, read-only:
 * verdict[s] (a device byte array of nstripes) is 1 exactly when
 * isParityCorrect(shards of stripe s, 0, byte_count) holds on the stripe's natural shards, else
 * 0.  block_bytes 0 = the recommended block.  One launch sets the verdicts, then the layout's two
 * passes clear them: a mismatch in any block of a stripe, or in its tail, clears that stripe's
 * byte.  Nothing is written to base.  nstripes == 0 touches nothing; byte_count == 0 makes every
 * verdict 1.  Status codes as ecx_rs_is_parity_correct_batch; a negative block_bytes is
 * ECX_E_ILLEGAL_ARGUMENT. */
int ecx_rs_is_parity_correct_blocked_batch(ecx_rs *rs, const uint8_t *base, int64_t nstripes, int64_t byte_count,
                                           int64_t block_bytes, uint8_t *verdict, void *stream);

/* Which shard is corrupt in a stripe that fails ReedSolomon.isParityCorrect
 * (ReedSolomon.java:129-178)?  The reference has no counterpart; this is the engine's, the step
 * between the scrub and the repair.  Layout of ecx_rs_is_parity_correct_batch, read-only, over bytes
 * [offset, offset + byte_count) of stripe s:
 *   suspect[s][j] (a device byte array [nstripes][n]) = 1 when replacing shard j alone can make the
 *                 stripe pass isParityCorrect, else 0;
 *   culprit[s]    (a device int32 array of nstripes) = -1: the stripe is clean, all n suspects are 1;
 *                 j: exactly one suspect; -2: no single shard explains the stripe, no suspect is 1;
 *   heal_id[s]    (a device byte array of nstripes, or NULL: not wanted) = j when culprit[s] == j,
 *                 else 255.
 * Pattern j of the set made from the n patterns "shard j missing" (1 - identity) rebuilds shard j,
 * and id 255 has no pattern there, so ecx_rs_decode_missing_batch_mixed(that set, heal_id, ...) on
 * the same stream heals the batch with no host round trip.  With H = [P | I] the m x n check matrix
 * and S(b) = H x(b) the syndromes at byte b, shard j explains the stripe exactly when S(b) is a
 * multiple of column H_j at every b; the kernel tests that on the syndromes the check already holds
 * in registers, so a clean stripe costs what the check costs.
 * What the answer means: with m = 2 two corrupt shards at the SAME byte position can imitate a
 * third shard (a CPU probe against the oracle's brute force saw it in 2 of 45 cases for RS(4,2) and
 * 6 of 30 for RS(3,2)), and healing then rewrites a good shard from bad ones.  For m >= 3 the probe
 * saw no such case: a code of distance m + 1 tells two errors from one.
 * ECX_E_ILLEGAL_ARGUMENT: m < 2 (every column matches every syndrome), m > 8 (the check map is no
 * longer one tile), heal_id wanted with n > 255, a negative count.  The pointers are checked after
 * the counts (ECX_E_NULL).  nstripes == 0 touches nothing; byte_count == 0 makes every stripe clean.
 * The first call of a codec on a device uploads its plans and must be made outside stream capture. */
int ecx_rs_locate_corrupt_batch(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                int64_t nstripes, int64_t offset, int64_t byte_count, uint8_t *suspect,
                                int32_t *culprit, uint8_t *heal_id, void *stream);
/* The same over the blocked layout (ecx_rs_is_parity_correct_blocked_batch's arguments; isParityCorrect,
 * ReedSolomon.java:129-178, on the stripe's natural shards over [0, byte_count)): the layout's two
 * passes clear the suspects of unit / full's stripe, so a shard stays a suspect when it explains
 * every block of its stripe and the tail.  heal_id feeds ecx_rs_decode_missing_blocked_batch_mixed. */
int ecx_rs_locate_corrupt_blocked_batch(ecx_rs *rs, const uint8_t *base, int64_t nstripes, int64_t byte_count,
                                        int64_t block_bytes, uint8_t *suspect, int32_t *culprit, uint8_t *heal_id,
                                        void *stream);

/* Which ONE OR TWO shards are corrupt?  ecx_rs_locate_corrupt_batch leaves a stripe with two corrupt
 * shards at culprit -2; a code with m >= 4 parity shards has distance m + 1 >= 5 and corrects two
 * errors.  Arguments and layout of ecx_rs_locate_corrupt_batch, read-only, with wider outputs:
 *   suspect[s]    (a device byte array [nstripes][n + C(n,2)]): the n single suspects as above, then
 *                 one byte per pair {i, j}, i < j, at n + p with p = i(2n - i - 1)/2 + (j - i - 1)
 *                 (lexicographic pair order): 1 when replacing shards i and j together can make the
 *                 stripe pass isParityCorrect, else 0;
 *   culprit[s]    (a device int32 array [nstripes][2]) and heal_id[s] (device bytes, or NULL):
 *                   all n singles set                        (-1, -1)   255
 *                   exactly one single, j                    (j, -1)    j
 *                   no single, exactly one pair p = {i, j}   (i, j)     n + p
 *                   anything else                            (-2, -2)   255
 * The pattern set of the n single-loss patterns in shard order followed by the C(n,2) pair-loss
 * patterns in pair order gives every heal id its pattern, so ecx_rs_decode_missing_batch_mixed on
 * the same stream heals the batch.  The pair {i, j} explains a stripe exactly when S(b) lies in
 * span(H_i, H_j) at every b: m - 2 test rows per pair on the syndromes the check holds in
 * registers.  Any four columns of H being independent for m >= 4, one corrupt shard i leaves
 * suspect i and the n - 1 pairs that contain i, and two corrupt shards i, j -- at the same byte or at
 * different ones -- leave no single suspect and the pair {i, j} alone.  A wave that keeps a single
 * candidate evaluates no pair row.
 * What the answer means: THREE corrupt shards can imitate a pair of other shards (3 + 2 >= m + 1
 * for m = 4), and healing then rewrites good shards from bad ones; DESIGN.md section 4.8.1 has the
 * measured rate.  Three or more corrupt shards are out of scope.
 * ECX_E_ILLEGAL_ARGUMENT: m < 4 (two errors need 2 * 2 <= m), m > 8, n > 64 (a wave holds one 64-bit
 * mask of single candidates), heal_id wanted with n + C(n,2) > 255 (n > 22), a negative count.  The
 * pointers are checked after the counts (ECX_E_NULL).  nstripes == 0 touches nothing; byte_count == 0
 * makes every stripe clean.  The first call of a codec on a device uploads its plans and must be
 * made outside stream capture. */
int ecx_rs_locate_corrupt2_batch(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                 int64_t nstripes, int64_t offset, int64_t byte_count, uint8_t *suspect,
                                 int32_t *culprit, uint8_t *heal_id, void *stream);
/* The same over the blocked layout, as ecx_rs_locate_corrupt_blocked_batch (and refusing what it
 * refuses); heal_id feeds ecx_rs_decode_missing_blocked_batch_mixed. */
int ecx_rs_locate_corrupt2_blocked_batch(ecx_rs *rs, const uint8_t *base, int64_t nstripes, int64_t byte_count,
                                         int64_t block_bytes, uint8_t *suspect, int32_t *culprit, uint8_t *heal_id,
                                         void *stream);

/* The same two blocked batches (encodeParity / decodeMissing, ReedSolomon.java:94-108, :189-286)
 * from HOST memory, in place (base: nstripes * n * byte_count bytes of
 * pageable or pinned host memory in the blocked layout): the full blocks, then the tails, each a
 * pipelined host batch (H2D -> map -> D2H of the written shards only, as ecx_map_apply_batch_host).
 * Synchronous; a caller that keeps its stripes blocked on the host feeds the device the layout
 * the kernels run fastest on without an unpacking pass. */
int ecx_rs_encode_parity_blocked_batch_host(ecx_rs *rs, uint8_t *base, int64_t nstripes, int64_t byte_count,
                                            int64_t block_bytes);
int ecx_rs_decode_missing_blocked_batch_host(ecx_rs *rs, const uint8_t *shard_present, uint8_t *base,
                                             int64_t nstripes, int64_t byte_count, int64_t block_bytes);
/* The same over several GPUs of this process: each of the two passes is split over the device
 * entries as ecx_map_apply_batch_host_devices splits a batch -- the full blocks as nstripes * full
 * small stripes, the tails by stripes (by byte ranges when there are fewer than entries). */
int ecx_rs_encode_parity_blocked_batch_host_devices(ecx_rs *rs, uint8_t *base, int64_t nstripes, int64_t byte_count,
                                                    int64_t block_bytes, const int *devices, int ndev);
int ecx_rs_decode_missing_blocked_batch_host_devices(ecx_rs *rs, const uint8_t *shard_present, uint8_t *base,
                                                     int64_t nstripes, int64_t byte_count, int64_t block_bytes,
                                                     const int *devices, int ndev);
/* ReedSolomon.isParityCorrect (ReedSolomon.java:129-178) over HOST-memory stripes in the blocked
 * layout (base: nstripes * n * byte_count bytes of pageable or pinned host memory, read-only;
 * verdict: nstripes host bytes), as ecx_rs_is_parity_correct_blocked_batch: each of the layout's
 * two passes is a pipelined host check (ecx_rs_is_parity_correct_batch_host) with one verdict
 * byte per unit of the pass, folded per stripe on the host -- about 1 verdict byte per
 * n * block_bytes data bytes.  Synchronous.  A store that keeps its stripes blocked scrubs them
 * without an unpacking pass. */
int ecx_rs_is_parity_correct_blocked_batch_host(ecx_rs *rs, const uint8_t *base, int64_t nstripes,
                                                int64_t byte_count, int64_t block_bytes, uint8_t *verdict);
/* ReedSolomon.isParityCorrect (ReedSolomon.java:129-178), the blocked host check over several
 * GPUs of this process: each pass is split over the device entries as
 * ecx_rs_is_parity_correct_batch_host_devices splits a check (the tails by byte ranges when
 * there are fewer stripes than entries).  The device list is validated even for an empty batch. */
int ecx_rs_is_parity_correct_blocked_batch_host_devices(ecx_rs *rs, const uint8_t *base, int64_t nstripes,
                                                        int64_t byte_count, int64_t block_bytes, uint8_t *verdict,
                                                        const int *devices, int ndev);

/* decodeMissing (ReedSolomon.java:189-286) per stripe over the blocked layout, in place: stripe s of
 * the nstripes stripes at base (body [nstripes][full][n][block], then tails [nstripes][n][tail];
 * block_bytes 0 = the recommended block) is decoded with pattern pattern_of_stripe[s], a DEVICE
 * byte array of nstripes.  An id with no pattern, or a pattern with nothing missing, leaves every
 * byte of that stripe untouched, body and tail.  Each pass of the layout is one launch; a block
 * row finds its stripe's id as unit / full on the device.  Only enqueues.  Checked in this order:
 * null set ECX_E_NULL; negative nstripes or byte_count ECX_E_ILLEGAL_ARGUMENT; null base or
 * pattern_of_stripe ECX_E_NULL; negative block_bytes or an extent beyond int64_t
 * ECX_E_ILLEGAL_ARGUMENT; nstripes == 0 or byte_count == 0 enqueues nothing. */
int ecx_rs_decode_missing_blocked_batch_mixed(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                              uint8_t *base, int64_t nstripes, int64_t byte_count,
                                              int64_t block_bytes, void *stream);
/* decodeMissing (ReedSolomon.java:189-286) per stripe over HOST-memory stripes, in place, layout
 * and meaning of ecx_rs_decode_missing_batch_mixed: base and pattern_of_stripe are host pointers
 * (pageable or pinned).  Synchronous, on the current device: the ids go to the device once, then
 * chunks of stripes are pipelined H2D -> mixed launch -> D2H.  D2H returns the union of the
 * patterns' output shards for every stripe, so H2D carries that union as well as every shard a
 * pattern reads (up to n shards up instead of k): a shard one pattern rebuilds comes back
 * unchanged for the stripes of the other patterns.  Present shards, untouched stripes and bytes
 * outside [offset, offset + byte_count) are bit-identical afterwards.  A batch of no stripes needs
 * no buffers; without a usable device a batch with work returns ECX_E_DEVICE. */
int ecx_rs_decode_missing_mixed_batch_host(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                           uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                           int64_t nstripes, int64_t offset, int64_t byte_count);
/* decodeMissing (ReedSolomon.java:189-286) per stripe over HOST-memory stripes in the blocked
 * layout, in place: ecx_rs_decode_missing_blocked_batch_mixed with host pointers, each pass of the
 * layout a pipelined host batch as ecx_rs_decode_missing_mixed_batch_host (the ids cross once for
 * both; a chunk of block rows may begin mid-stripe).  Synchronous, on the current device. */
int ecx_rs_decode_missing_blocked_mixed_batch_host(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                                   uint8_t *base, int64_t nstripes, int64_t byte_count,
                                                   int64_t block_bytes);

/* As ecx_map_apply_batch, but XOR-accumulates: out ^= M * in. */
int ecx_map_accumulate_batch(const ecx_map *map, const uint8_t *in, int64_t in_stripe_stride,
                             int64_t in_slot_stride, uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride,
                             int64_t nstripes, int64_t byte_count, void *stream);

/* Maps of the codec entry points (owned by the codec; do not destroy). */
int ecx_rs_encode_map(ecx_rs *rs, const ecx_map **out);              /* encodeParity, slots = shard index */
int ecx_rs_decode_map(ecx_rs *rs, const uint8_t *shard_present, const ecx_map **out); /* decodeMissing */

/* ---------------------------------------------------------------- batched partial sums (repair pipelining) */
/* Batched ReedSolomon.decodeMissingSingle (ReedSolomon.java:288-333) as used along the
 * pipelined chain (ClayCodeNode.kt:182-186, :225-228): one helper's contribution to EVERY
 * missing shard, over nstripes stripes: acc[s][o] (=, or ^= unless is_first)
 * D[o][shard_index] * in[s], with o over the missing shards in ascending index order.
 * Unlike the reference (bug B3) the rows include missing PARITY shards (the composed
 * decodeMissing map), so a parity-node repair can be pipelined too.  A present shard that
 * is not among the first k present contributes zero (the reference's first-k rule). */
int ecx_rs_decode_partial_batch(ecx_rs *rs, const uint8_t *shard_present, int shard_index, const uint8_t *in,
                                int64_t in_stripe_stride, uint8_t *acc, int64_t acc_stripe_stride,
                                int64_t acc_row_stride, int64_t nstripes, int64_t byte_count, int is_first,
                                void *stream);
/* Batched ReedSolomon.decodeMissingSingle (ReedSolomon.java:288-333) with a pattern and a helper
 * shard index per stripe: the hop of the pipelined chain (ClayCodeNode.kt:165-193) for a store
 * whose placement rotates, so that both the stripe's missing shards and the shard this helper
 * holds change from stripe to stripe.  pattern_of_stripe and shard_of_stripe are DEVICE byte
 * arrays of nstripes.  For stripe s with p = pattern_of_stripe[s] and i = shard_of_stripe[s] the
 * input is in + s * in_stripe_stride + i * in_shard_stride (in_shard_stride 0: the helper's own
 * shards back to back; non-zero: shard i of a full stripe), and acc[s][o] (=, or ^= unless
 * is_first) D_p[o][i] * input for o over pattern p's missing shards in ascending order -- bit for
 * bit what ecx_rs_decode_partial_batch(rs, pattern p, i, ...) gives for that stripe: data and
 * parity rows, the first-k rule, zero from a shard pattern p does not read.  Rows at or past
 * pattern p's missing count are untouched; a stripe whose id has no pattern, whose pattern misses
 * nothing, or whose shard byte is >= n is untouched entirely, also with is_first.  Whatever the two
 * arrays hold, nothing outside the plan and the stripe's own input is read.  in and acc must not
 * overlap.  Only enqueues; the first use of a set on a device uploads its partial-sum plan
 * (npatterns * n * 192 bytes) and must happen outside stream capture (refused under capture,
 * nothing enqueued).  Checked in this order: null set ECX_E_NULL; negative nstripes or byte_count
 * ECX_E_ILLEGAL_ARGUMENT; nstripes == 0, byte_count == 0 or a set whose patterns miss nothing
 * ECX_OK (no buffers, no device); a null pointer among the four ECX_E_NULL; a negative stride or
 * an extent beyond int64_t ECX_E_ILLEGAL_ARGUMENT. */
int ecx_rs_decode_partial_batch_mixed(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                      const uint8_t *shard_of_stripe, const uint8_t *in, int64_t in_stripe_stride,
                                      int64_t in_shard_stride, uint8_t *acc, int64_t acc_stripe_stride,
                                      int64_t acc_row_stride, int64_t nstripes, int64_t byte_count, int is_first,
                                      void *stream);
/* Batched ReedSolomon.encodeParitySingle (ReedSolomon.java:110-118; LRC chains,
 * NodeHelper.kt:89): acc[s][p] (=, or ^= unless is_first) parityRows[p][input_index] * in[s]
 * for every parity row p. */
int ecx_rs_encode_partial_batch(ecx_rs *rs, int input_index, const uint8_t *in, int64_t in_stripe_stride,
                                uint8_t *acc, int64_t acc_stripe_stride, int64_t acc_row_stride, int64_t nstripes,
                                int64_t byte_count, int is_first, void *stream);

/* ---------------------------------------------------------------- ClayCodeErasureDecodingStep.java */
typedef struct ecx_clay ecx_clay;
/* new ClayCodeErasureDecodingStep(erasedIndexes, RS(2,2), RS(k,m)) -- ClayCode.java:28-41, :43-51 */
int ecx_clay_create(int data_units, int parity_units, const int *erased, int n_erased, ecx_clay **out);
/* Shortened Clay: Clay(data+virtual, parity) whose data nodes
 * [data, data+virtual) are virtual all-zero nodes, e.g. Clay(10,4) = Clay(12,4)
 * with 2 virtual nodes (the reference's integer t = (k+m)/m cannot build
 * Clay(10,4), ClayCodeErasureDecodingStep.java:692).  Every slot index, erased
 * index and geometry query then refers to the data+parity REAL nodes; the
 * results equal the reference Clay(12,4) run with the virtual nodes zero-filled. */
int ecx_clay_create_shortened(int data_units, int parity_units, int virtual_units, const int *erased, int n_erased,
                              ecx_clay **out);
/* ecx_clay_create_shortened with flags.  ECX_CLAY_IS_TEST: the single-node repair's plane
 * decode takes decodeDecoupledPlane's -DisTest=true branch (ClayCodeErasureDecodingStep.java:
 * 571-581): decodeMissingSingle per helper, assuming the erased row is nodes 0..q-1 (bug B2).
 * For the other rows it computes the reference's (different) map, and where that row holds a
 * parity node the reference throws NullPointerException (B3): ECX_E_NULL from performCoding.
 * Multi-erasure decodes (and encode) are unaffected, as in the reference. */
enum { ECX_CLAY_IS_TEST = 1 };
int ecx_clay_create_ex(int data_units, int parity_units, int virtual_units, const int *erased, int n_erased, int flags,
                       ecx_clay **out);
void ecx_clay_destroy(ecx_clay *clay); /* drops one reference (see ecx_rs_create) */
int ecx_clay_geometry(const ecx_clay *clay, int *q, int *t, int *alpha); /* ClayCodeUtil :690-695 */
int ecx_clay_helper_planes(const ecx_clay *clay, int erased_index, int *out /* alpha */); /* :924-941 */
/* The step's real node count n (= data + parity; virtual nodes excluded), its number of
 * erased nodes and alpha: performCoding takes n*alpha inputs and n_erased*alpha outputs
 * (the "Invalid inputs/outputs length" checks, ClayCodeErasureDecodingStep.java:76-82). */
int ecx_clay_shape(const ecx_clay *clay, int *nodes, int *n_erased, int *alpha);
/* performCoding(ECChunk[],ECChunk[]) -- ClayCodeErasureDecodingStep.java:53-107.
 * inputs: n*alpha host pointers, NULL = absent; outputs: n_erased*alpha host pointers. */
int ecx_clay_perform_coding(ecx_clay *clay, const uint8_t *const *inputs, uint8_t *const *outputs, int buf_size);
/* doDecodeSingle overload 2 (:225-282), as driven per helper plane by
 * ClayCodeHelper.getHelperPlanesAndDecode (ClayCodeHelper.kt:19-56).
 * helper_coupled: [num_helper_planes][n] host pointers; outputs: alpha host pointers. */
int ecx_clay_decode_single_helper(ecx_clay *clay, const uint8_t *const *helper_coupled, int helper_i,
                                  uint8_t *const *outputs, int erased_index, int buf_size);
/* The composed performCoding map for the standard null pattern (erased nodes
 * absent, every other sub-chunk present): input slot z*n+node, output slot z*|E|+j. */
int ecx_clay_map(ecx_clay *clay, const ecx_map **out);
/* Batched device-resident performCoding over nstripes stripes: stripe s holds
 * n*alpha sub-chunks of buf_size bytes at in + s*in_stripe_stride + slot*in_sub_stride
 * and receives |E|*alpha sub-chunks at out + s*out_stripe_stride + slot*out_sub_stride. */
int ecx_clay_perform_coding_batch(ecx_clay *clay, const uint8_t *in, int64_t in_stripe_stride,
                                  int64_t in_sub_stride, uint8_t *out, int64_t out_stripe_stride,
                                  int64_t out_sub_stride, int64_t nstripes, int64_t buf_size, void *stream);
/* isParityCorrect for Clay stripes: whether each of nstripes device-resident stripes of the
 * geometry ecx_clay_create_shortened(data_units, parity_units, virtual_units, ...) is still a
 * codeword, in one read-only launch (k_clay_check; geometries of at most 16 syndrome rows, Clay(2,2)
 * and Clay(4,2), run their dense syndrome map on k_gf_check instead, which measured faster there).
 * The layout is ecx_clay_perform_coding_batch's input layout: real slot z*n + node (n = data_units + parity_units real nodes, virtual nodes hold
 * no slot) of stripe s lies at base + s*stripe_stride + slot*sub_stride and is buf_size bytes long.
 * verdict is a device byte array of nstripes.
 * verdict[s] == 1 means: over bytes [0, buf_size) of every sub-chunk, the parity nodes of stripe s
 * are exactly what encoding its data nodes gives -- the stripe is a codeword.  It is a codeword
 * test and nothing more: a 0 does not say which node is corrupt, nor how many are, and a 1 says
 * nothing about bytes past buf_size (the padding of a layout with sub_stride > buf_size).
 * The call only enqueues on `stream` and writes nothing but verdict.
 * Checked in this order: negative counts ECX_E_ILLEGAL_ARGUMENT; nstripes == 0 returns ECX_OK with
 * nothing touched; null base or verdict ECX_E_NULL; a negative stride, or an extent beyond int64_t,
 * ECX_E_ILLEGAL_ARGUMENT.  buf_size == 0 makes every stripe pass.
 * Geometries: every one ecx_clay_create_shortened accepts whose nodes fill the q x t grid, with
 * parity_units <= 8 (one accumulator tile), and whose check program the planner can prove (every
 * encoded stripe has zero syndromes, and only those); any other is refused with
 * ECX_E_ILLEGAL_ARGUMENT and the reason in ecx_last_error.  The proof runs on the geometry's first
 * call in the process (about 0.1 s for Clay(12,4)) and is kept with the shared codec.
 * The first call for a geometry on a device uploads its node records and must be made outside
 * stream capture (under capture it returns ECX_E_DEVICE and leaves no node behind); later calls
 * may be captured and replayed.
 * Lifetime: the proved program and its device records belong to the shared codec of the geometry,
 * the object ecx_clay_create_shortened(data_units, parity_units, virtual_units, NULL, 0, &h)
 * returns.  The call itself holds that codec only while it runs; afterwards the codec is idle and
 * may be evicted (its device records freed) once 64 other codecs have been released.  A caller who
 * checks repeatedly should hold such a handle between calls, so the proof and the upload are paid
 * once; a caller who CAPTURES the call MUST hold one from before the warm-up call until the graph
 * is destroyed, because the graph's kernel nodes keep pointers to those records, and must not
 * destroy it while enqueued work is in flight.  The Python and Java wrappers hold it for you. */
int ecx_clay_is_parity_correct_batch(int data_units, int parity_units, int virtual_units, const uint8_t *base,
                                     int64_t stripe_stride, int64_t sub_stride, int64_t nstripes, int64_t buf_size,
                                     uint8_t *verdict, void *stream);

/* A Clay pattern set -- performCoding (ClayCodeErasureDecodingStep.java:53-107) over a batch whose
 * stripes lost DIFFERENT nodes, in one launch.  The set holds up to 256 erased-node lists of one
 * geometry as one device plan; list p is the standard-null-pattern performCoding map of
 * ecx_clay_create_ex(data_units, parity_units, virtual_units, list p, 0): input slot z*n + node,
 * output slot z*|E_p| + j.  `erased` holds the lists back to back, n_erased[p] entries for list p.
 * An empty list is the "nothing erased" pattern and does nothing; duplicate lists are allowed.
 * The set holds one codec reference per distinct list and drops them in destroy.
 * Refused: npatterns outside 1..256 (ECX_E_ILLEGAL_ARGUMENT); a list the single step refuses (that
 * step's own status).
 * A GENERATED set: the geometries with 256 rows per node, Clay(12,4) and the shortened Clay(10,4),
 * have maps too tall for the device plan (more than 64 rows).  A set whose non-empty lists are all
 * single nodes of such a geometry with q = 4 and t >= 3 is accepted and runs on a kernel generated
 * for the set and compiled at run time with hiprtc (k_clay_repair_set: one straight-line body per
 * distinct list, chosen per stripe by its id byte).  The first batch of such a set on a device
 * compiles and loads it (a few tenths of a second per body) and must run outside stream capture; without hiprtc
 * that batch returns ECX_E_DEVICE with the reason -- no other kernel can run these maps.
 * Still refused with ECX_E_ILLEGAL_ARGUMENT, naming the list, its row count and
 * ecx_clay_perform_coding_batch (repair such stripes with it, one list per call): a list of more
 * than 64 rows that erases several nodes; a single-node list of more than 64 rows of a geometry
 * without that kernel (Clay(9,3): 81 rows, q = 3); generated and plan lists mixed in one set. */
typedef struct ecx_clay_pattern_set ecx_clay_pattern_set;
int ecx_clay_pattern_set_create(int data_units, int parity_units, int virtual_units,
                                const int *erased /* the lists back to back */,
                                const int *n_erased /* npatterns counts */, int npatterns,
                                ecx_clay_pattern_set **out);
/* Frees the set and its device plans (ClayCodeErasureDecodingStep.java:53-107 has no counterpart:
 * the reference builds one step per repair).  NULL is ignored. */
void ecx_clay_pattern_set_destroy(ecx_clay_pattern_set *set);
/* The set's list count, the step's real node count n, alpha, and the most nodes any list erases
 * (the shape checks of ClayCodeErasureDecodingStep.java:53-107: a stripe takes n*alpha inputs
 * and up to max_erased*alpha outputs).  Each out pointer may be NULL. */
int ecx_clay_pattern_set_info(const ecx_clay_pattern_set *set, int *npatterns, int *nodes, int *alpha,
                              int *max_erased);
/* performCoding (ClayCodeErasureDecodingStep.java:53-107) with a list per stripe, in the layout of
 * ecx_clay_perform_coding_batch: stripe s is repaired with list pattern_of_stripe[s] (a DEVICE
 * byte array of nstripes, read by the kernel) and receives output slots 0 .. |E_p|*alpha - 1.
 * Left untouched: the slots past that; every slot of a stripe whose id has no list or whose list is
 * empty; every byte outside [0, buf_size) of a slot.  `in` and `out` must not overlap.  The call
 * only enqueues.  Checked in this order: a null set (ECX_E_NULL); negative nstripes or buf_size
 * (ECX_E_ILLEGAL_ARGUMENT); nstripes == 0, buf_size == 0 or a set whose lists are all empty
 * (ECX_OK: no buffer is looked at, no device needed); a null pointer among the three (ECX_E_NULL);
 * a negative stride or an extent beyond int64_t (ECX_E_ILLEGAL_ARGUMENT).
 * A generated set (above) covers whole 4 KiB chunks of 16-byte-aligned layouts and has no kernel
 * for a tail, so after the checks above and before any device work it also refuses, with
 * ECX_E_ILLEGAL_ARGUMENT and the offending value in the message: a buf_size that is not a multiple
 * of 4096; a base or a stride that is not a multiple of 16 (Clay(10,4)'s sub-chunks are 4 KiB or
 * 1 MiB; slot offsets beyond 31 bits take the kernel's 64-bit-address form).  The host form
 * below stages every slot itself and has the buf_size rule only. */
int ecx_clay_perform_coding_batch_mixed(const ecx_clay_pattern_set *set,
                                        const uint8_t *pattern_of_stripe /* device */, const uint8_t *in,
                                        int64_t in_stripe_stride, int64_t in_sub_stride, uint8_t *out,
                                        int64_t out_stripe_stride, int64_t out_sub_stride, int64_t nstripes,
                                        int64_t buf_size, void *stream);
/* One hop of the pipelined Clay repair chain (ClayCoordinator.kt:265-319 starts the chain,
 * ClayCodeNode.kt:165-233 is a helper's step: add its share to the partial sum and forward it)
 * with an erased-node list AND the node this helper holds per stripe: the deployment of one helper
 * per machine under rotating placement, in one launch.  pattern_of_stripe and node_of_stripe are
 * DEVICE byte arrays of nstripes.  For stripe s with p = pattern_of_stripe[s] and
 * i = node_of_stripe[s], plane z of the helper's node lies at
 * in + s * in_stripe_stride + i * in_node_stride + z * in_sub_stride (in_node_stride 0: the
 * helper's own sub-chunks back to back, the node-major local layout; in_node_stride = sub and
 * in_sub_stride = n * sub: node i inside a full plane-major stripe).  With M_p list p's map of
 * ecx_clay_pattern_set_create (input slot z*n + node, output slot z*|E_p| + j), every row
 * r in 0 .. |E_p|*alpha - 1 at acc + s * acc_stripe_stride + r * acc_sub_stride is assigned
 * (is_first) or XORed with sum_z M_p[r][z*n + i] * in(s, z) -- bit for bit what
 * ecx_map_accumulate_batch (ecx_map_apply_batch when is_first) gives for that stripe with the
 * columns of node i of list p's map, so the hops of all n nodes sum to
 * ecx_clay_perform_coding_batch_mixed.  A node list p does not read -- an erased node, or planes
 * the single-node repair skips -- adds nothing to a running sum and assigns zeros to the list's
 * rows with is_first.  Rows at or past |E_p|*alpha are untouched; a stripe whose id has no list,
 * whose list is empty or whose node byte is >= n is untouched entirely, also with is_first.
 * Whatever the two arrays hold, nothing outside the plan and the stripe's own node input is read.
 * in and acc must not overlap.  Only enqueues; the first use of a set on a device uploads its
 * partial-sum plan (256 * n * T tile records of 64 bytes, T the set's tiles per list, and 192
 * bytes per ring-padded entry: 96 KiB + 22.5 KiB for the six single-node lists of Clay(4,2)) and
 * must happen outside stream capture (refused under capture, nothing enqueued).  Checked in this
 * order: null set ECX_E_NULL; negative nstripes or buf_size ECX_E_ILLEGAL_ARGUMENT; nstripes == 0,
 * buf_size == 0 or a set whose lists are all empty ECX_OK (no buffers, no device); a null pointer
 * among the four ECX_E_NULL; a negative stride or an extent beyond int64_t
 * ECX_E_ILLEGAL_ARGUMENT.  A generated set (ecx_clay_pattern_set_create) has no partial-sum hop
 * yet: it is refused by name (ECX_E_ILLEGAL_ARGUMENT) right after the null-set check. */
int ecx_clay_partial_batch_mixed(const ecx_clay_pattern_set *set,
                                 const uint8_t *pattern_of_stripe /* device */,
                                 const uint8_t *node_of_stripe /* device */, const uint8_t *in,
                                 int64_t in_stripe_stride, int64_t in_node_stride, int64_t in_sub_stride,
                                 uint8_t *acc, int64_t acc_stripe_stride, int64_t acc_sub_stride,
                                 int64_t nstripes, int64_t buf_size, int is_first, void *stream);

/* ---------------------------------------------------------------- LRC (device batch, in place) */
/* LRCErasureCode.kt:5-9 / LRCErasureUtil.kt:3-6: K=12 data blocks in local groups of
 * R=3, one RS(3,1) parity each (parity row [1,1,1], i.e. XOR), N=16 blocks in the
 * LRCErasureCodeExample.kt:48 order (group g = blocks 4g..4g+3, parity 4g+3).
 * Block b of stripe s is at stripes + s*stripe_stride + b*block_stride. */
/* The composed map: block_present == NULL -> encode, else decode (owned by the library). */
int ecx_lrc_map(const uint8_t *block_present /* 16 flags or NULL */, const ecx_map **out);
/* encode / encodeUsingSingle (LRCErasureCodeExample.kt:30-98): writes the 4 group parities. */
int ecx_lrc_encode_batch(uint8_t *stripes, int64_t stripe_stride, int64_t block_stride, int64_t nstripes,
                         int64_t block_size, void *stream);
/* decode (LRCErasureCodeExample.kt:100-131): rebuilds every non-present block from
 * its group (decodeMissing per group).  Two blocks missing in one group ->
 * ECX_E_NOT_ENOUGH_SHARDS, as RS(3,1).decodeMissing throws. */
int ecx_lrc_decode_batch(uint8_t *stripes, int64_t stripe_stride, int64_t block_stride,
                         const uint8_t *block_present /* 16 flags */, int64_t nstripes, int64_t block_size,
                         void *stream);

/* ---------------------------------------------------------------- host-memory batches */
/* The reference's repair starts and ends in host memory: helper sub-chunks arrive on
 * sockets into ByteBuffers (ClayCoordinator.kt:372-395) and leave the same way
 * (ClayCodeNode.kt:330-347).  A JNI shim hands over their addresses via
 * GetDirectBufferAddress (ECChunk.toBuffers, ECChunk.java:81-95).
 * These calls take the batch layouts above with HOST pointers.  Chunks of stripes are
 * pipelined H2D -> kernel -> D2H on internal streams, and only the map's used input
 * slots cross PCIe.  The calls are synchronous.  Pinned memory (ecx_host_alloc /
 * ecx_host_register) runs at the PCIe rate.  Outputs may point into the input stripes
 * (in-place decodeMissing) when no output slot is also an input slot. */
int ecx_map_apply_batch_host(const ecx_map *map, const uint8_t *in, int64_t in_stripe_stride,
                             int64_t in_slot_stride, uint8_t *out, int64_t out_stripe_stride,
                             int64_t out_slot_stride, int64_t nstripes, int64_t byte_count);
int ecx_clay_perform_coding_batch_host(ecx_clay *clay, const uint8_t *in, int64_t in_stripe_stride,
                                       int64_t in_sub_stride, uint8_t *out, int64_t out_stripe_stride,
                                       int64_t out_sub_stride, int64_t nstripes, int64_t buf_size);
/* The same over several GPUs of this process (one host thread, stream set and
 * buffer ring per GPU).  Device j of `devices` (ndev entries, HIP ordinals; repeats allowed)
 * takes the contiguous stripe range [j*S/ndev, (j+1)*S/ndev) (the remainder spread over the
 * first ranges, as shard_stripes), on a worker thread of its own; the call returns when every
 * worker has finished.  With fewer stripes than entries (one or two huge stripes) the entries
 * split the bytes of every slot instead, in 4 KiB units, so each still moves a share over its
 * own link.  An out-of-range device id or ndev <= 0 is refused
 * (ECX_E_ILLEGAL_ARGUMENT) before anything is copied; on a failure every device is drained and
 * the first failing device's status is returned.  The calling thread's current device is
 * unchanged. */
int ecx_map_apply_batch_host_devices(const ecx_map *map, const uint8_t *in, int64_t in_stripe_stride,
                                     int64_t in_slot_stride, uint8_t *out, int64_t out_stripe_stride,
                                     int64_t out_slot_stride, int64_t nstripes, int64_t byte_count,
                                     const int *devices, int ndev);
int ecx_clay_perform_coding_batch_host_devices(ecx_clay *clay, const uint8_t *in, int64_t in_stripe_stride,
                                               int64_t in_sub_stride, uint8_t *out, int64_t out_stripe_stride,
                                               int64_t out_sub_stride, int64_t nstripes, int64_t buf_size,
                                               const int *devices, int ndev);
/* ecx_clay_perform_coding_batch_mixed (performCoding, ClayCodeErasureDecodingStep.java:53-107,
 * with a list per stripe) over HOST memory: `pattern_of_stripe`, `in` and `out` are host pointers.
 * Synchronous, on the current device.  The ids cross once; chunks of stripes then go H2D (the union
 * of the lists' input slots), through the mixed launch and D2H.  The pipeline cannot know a
 * stripe's list, so output slots 0 .. max_p |E_p|*alpha - 1 come back for EVERY stripe, and the part
 * a stripe's own list does not write comes back as ZEROS: the slots past |E_p|*alpha, and all of
 * them for a stripe whose id has no list or whose list is empty.  This is the one place where the
 * host form differs from the device form, which leaves those bytes untouched.  Host bytes outside
 * the returned slots and outside [0, buf_size) of a slot are untouched.  The checks and their
 * order are the device form's.  There is no _host_devices form.  A generated set
 * (ecx_clay_pattern_set_create) runs the same ring with k_clay_repair_set as its launch: the union
 * of its lists' helper planes goes up (all 3,584 slots of a stripe for the 14 single-node lists of
 * Clay(10,4)), slots 0 .. alpha - 1 come back, the zero rule is unchanged, and buf_size must be a
 * multiple of 4096 (the staging buffers give the alignment the kernel needs). */
int ecx_clay_perform_coding_mixed_batch_host(const ecx_clay_pattern_set *set,
                                             const uint8_t *pattern_of_stripe /* host */, const uint8_t *in,
                                             int64_t in_stripe_stride, int64_t in_sub_stride, uint8_t *out,
                                             int64_t out_stripe_stride, int64_t out_sub_stride,
                                             int64_t nstripes, int64_t buf_size);
/* How ecx_clay_perform_coding_mixed_batch_host would move this batch of performCoding calls
 * (ClayCodeErasureDecodingStep.java:53-107; host-only, no device touched): plan[7] = {input slots
 * that go up per stripe (the union of the lists' input slots), output slots that come back per
 * stripe (0 .. max |E|*alpha - 1), stripes per pipelined chunk, chunks, device buffer sets in
 * flight, H2D copies per chunk, D2H copies per chunk}.  All zero when the batch moves nothing (no
 * stripes, no bytes, a set whose lists are all empty). */
int ecx_clay_pattern_set_host_plan(const ecx_clay_pattern_set *set, int64_t in_stripe_stride,
                                   int64_t in_sub_stride, int64_t out_stripe_stride, int64_t out_sub_stride,
                                   int64_t nstripes, int64_t buf_size, int64_t *plan);
/* ReedSolomon.isParityCorrect (ReedSolomon.java:129-178) over nstripes HOST-memory stripes
 * (the layout of ecx_rs_is_parity_correct_batch, host pointers): each chunk of stripes goes
 * H2D and through the read-only check kernel, and only the verdict bytes come back --
 * verdict[s] (a host byte array of nstripes) = 1 when stripe s's parity is correct over bytes
 * [offset, offset + byte_count), else 0.  Synchronous; the _devices form splits the stripes
 * over a device list as ecx_map_apply_batch_host_devices does; with fewer stripes than entries
 * each entry checks a byte range of every shard, and a stripe passes when every range does. */
int ecx_rs_is_parity_correct_batch_host(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride,
                                        int64_t shard_stride, int64_t nstripes, int64_t offset,
                                        int64_t byte_count, uint8_t *verdict);
int ecx_rs_is_parity_correct_batch_host_devices(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride,
                                                int64_t shard_stride, int64_t nstripes, int64_t offset,
                                                int64_t byte_count, uint8_t *verdict, const int *devices,
                                                int ndev);
/* Page-locked host memory for the calls above (e.g. backing direct ByteBuffers). */
int ecx_host_alloc(int64_t nbytes, void **out);
int ecx_host_free(void *ptr);
int ecx_host_register(void *ptr, int64_t nbytes);
int ecx_host_unregister(void *ptr);

/* ---------------------------------------------------------------- synthetic data / verification (device) */
/* Deterministic counter-based fill: byte i of the region = f(seed, i). */
int ecx_fill_random(uint8_t *dst, int64_t nbytes, uint64_t seed, void *stream);
/* Count bytes that differ between two strided sets of nrows rows of row_bytes each;
 * result accumulated into *d_count (device uint64). */
int ecx_count_mismatch(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t nrows,
                       int64_t row_bytes, uint64_t *d_count, void *stream);

#ifdef __cplusplus
}
#endif
#endif
