/*
 * fhe_gpu.h — C ABI of the MI355X RNS-CKKS ciphertext-op engine that runs the
 * rank-sort / comparator hot path of oksuman/FHE-Sorting.
 *
 * Drop-in boundary.  In the reference every call below is a method of
 * OpenFHE's CryptoContext<DCRTPoly> reached from the sort code; this header
 * is what that code binds instead (C++ callers can also use the header-only
 * mirror in fhe-sorting_amd/csrc/algo/fhesort.hpp).  Each entry point names
 * the reference call site(s) it replaces.
 *
 * Rules: handles are opaque; every function returns an int status (FHE_OK =
 * 0); no C++ exception crosses the ABI (fhe_last_error() has the message);
 * results are new objects returned through **out and owned by the caller
 * (free with fhe_ct_free / fhe_pt_free); one context per GPU, calls on one
 * context must be serialised by the caller (the reference's OpenMP threads
 * share one CryptoContext; here one process drives one GPU).  All arrays are
 * host memory unless a name says `dev`.
 */
#ifndef FHE_GPU_H
#define FHE_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    FHE_OK = 0,
    FHE_EINVAL = 1,    /* bad argument / level mismatch / unsupported N */
    FHE_ENOKEY = 2,    /* rotation index without a key (OpenFHE throws in EvalRotate) */
    FHE_EDEPTH = 3,    /* no modulus levels left */
    FHE_EHIP = 4,      /* HIP runtime error */
    FHE_ENOMEM = 5,
    FHE_EINTERNAL = 6,
    FHE_ENOCOMM = 7,   /* collective requested without fhe_comm_init */
    FHE_EIO = 8        /* file cannot be read / written, or is not a valid wire file */
};

typedef struct fhe_ctx fhe_ctx;
typedef struct fhe_ct fhe_ct;
typedef struct fhe_pt fhe_pt;
typedef struct fhe_boot fhe_boot;

/* CCParams<CryptoContextCKKSRNS> subset used by the sort path
 * (tests/DirectSortTest.cpp:24-31; src/sort_algo.h:87-201) */
typedef struct {
    int log_n;       /* ring dimension 2^log_n (SetRingDim) */
    int mult_depth;  /* SetMultiplicativeDepth: mult_depth+1 Q primes */
    int scale_bits;  /* SetScalingModSize */
    int first_bits;  /* first modulus size (OpenFHE default 60) */
    int dnum;        /* hybrid key-switching digits (OpenFHE default 3) */
    uint64_t seed;   /* 0: the secret, every error and the encryption randomness are
                        drawn from ChaCha20 keyed by the OS CSPRNG (getrandom) -- use
                        this to protect data.  Nonzero: reproducible SplitMix64 streams
                        keyed by the seed (tests, parity with the CPU oracle); anyone
                        who knows the seed can regenerate the secret key.  The seed is
                        never written to a file (fhe_serialize_context writes 0). */
} fhe_params;

const char *fhe_last_error(void);
/* the secure sampler's block function (ChaCha20, RFC 8439 §2.3): 16 output
 * words for (key, counter, nonce).  Host-only, for known-answer tests. */
int fhe_prng_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]);

/* ---------------------------------------------------------------- context */
/* replaces GenCryptoContext(parameters) (tests/DirectSortTest.cpp:33).
 * The envelope: parameters the kernels cannot serve are refused with
 * FHE_EINVAL before the device is touched, *out stays NULL and fhe_last_error
 * names the parameter:
 *   log_n       10..17 (the wire format's range);
 *   mult_depth  >= 1;
 *   dnum        >= 1, with alpha = ceil((mult_depth + 1) / dnum) primes per
 *               digit: at most 8 digits at the top level
 *               (ceil((mult_depth + 1) / alpha) <= 8), alpha <= 24, and at most
 *               16 special primes (K = ceil((bits of the widest digit +
 *               log2 alpha) / 60)) -- raise dnum when a digit is too wide;
 *   scale_bits  20..59, first_bits scale_bits + 1 .. 60.
 * fhe_deserialize_context holds a context file to the same envelope.
 * fhe_params_check is the predicate alone (host arithmetic, no device): FHE_OK
 * and the context's Q primes, special primes, digit width and top-level digit
 * count (each pointer may be NULL), or FHE_EINVAL as above. */
int fhe_params_check(const fhe_params *p, int *nq, int *K, int *alpha, int *digits);
int fhe_ctx_create(const fhe_params *p, int device, fhe_ctx **out);
int fhe_ctx_destroy(fhe_ctx *ctx);
/* primes: nq+K values; deltas: mult_depth+1 canonical scales */
int fhe_ctx_info(fhe_ctx *ctx, int *nq, int *K, int *alpha, uint64_t *primes, double *deltas);
/* directory holding doubled_sinc_<N>.f64 (generated_doubled_sinc_coeffs.h) */
int fhe_set_coeff_dir(const char *dir);

/* ------------------------------------------------------------------- keys */
/* KeyGen + EvalMultKeyGen (tests/DirectSortTest.cpp:41-47), on the GPU */
int fhe_keygen(fhe_ctx *ctx);
/* EvalRotateKeyGen(sk, rotations) (tests/DirectSortTest.cpp:46) */
int fhe_gen_rotation_keys(fhe_ctx *ctx, const int32_t *idx, int n);
/* externally generated keys (identical layout to the CPU oracle):
 * secret [nq+K][n] NTT, public [2][nq][n], key [digits][2][nq+K][n] */
int fhe_ctx_load_secret(fhe_ctx *ctx, const uint64_t *s_ntt);
int fhe_ctx_load_public(fhe_ctx *ctx, const uint64_t *pk);
int fhe_ctx_load_keys(fhe_ctx *ctx, const uint64_t *relin, const int32_t *rot_idx,
                      const uint64_t *const *rot_keys, int nrot);
uint64_t fhe_key_bytes(fhe_ctx *ctx);
/* Seeded switching keys.  Half of every switching key is the public uniform
 * polynomial a_j; under a public seed keygen expands it on the GPU from a
 * counter-based ChaCha20 stream ("public stream v1", csrc/wire/wire.hpp) instead
 * of sampling it on the host, and the key can be written without that half
 * (fhe_serialize_eval_*_key_seeded below).  The secret, the errors and the
 * public key do not depend on it; without a public seed every key is what it
 * was before. */
/* public seed of the switching keys' uniform halves; NULL draws one from the OS CSPRNG,
   allowed only on a secure context (params.seed == 0): a test context must be given an
   explicit seed so nothing derived from the test seed can reach a file (else FHE_EINVAL).
   Affects keys generated afterwards. */
int fhe_set_public_seed(fhe_ctx *ctx, const uint8_t seed[32]);
int fhe_get_public_seed(fhe_ctx *ctx, uint8_t seed[32]);          /* FHE_EINVAL if none */
int fhe_key_is_seeded(fhe_ctx *ctx, uint64_t galois /* 0 = eval-mult */);  /* 1 / 0, < 0 no such key */

/* ------------------------------------------------------ ciphertext / pt */
/* Encryption::encryptInput = MakeCKKSPackedPlaintext + Encrypt (src/encryption.cpp:5-12) */
int fhe_encrypt(fhe_ctx *ctx, const double *v, int len, int slots, int level, fhe_ct **out);
/* the same under OpenFHE's default FLEXIBLEAUTOEXT scaling (the reference's MEHP24
 * tests, tests/mehp24/Mehp24SortTest.cpp:25-70, leave it at that default): one extra
 * level, consumed at encryption, divides the encryption noise by the top prime; the
 * ciphertext starts at level 1.  Build the context with multDepth + 1 levels. */
int fhe_encrypt_ext(fhe_ctx *ctx, const double *v, int len, int slots, fhe_ct **out);
/* DebugEncryption::getPlaintext / Decrypt (src/encryption.cpp:14-27); out: slots values */
int fhe_decrypt(fhe_ctx *ctx, const fhe_ct *ct, double *out);
int fhe_ct_upload(fhe_ctx *ctx, const uint64_t *host, int limbs, int level, int slots, double scale,
                  fhe_ct **out);
int fhe_ct_download(fhe_ctx *ctx, const fhe_ct *ct, uint64_t *host); /* [2][limbs][n] */
int fhe_ct_info(const fhe_ct *ct, int *level, int *slots, double *scale, int *limbs);
/* Ciphertext::SetSlots (src/sort_algo.h:429,447,501) */
int fhe_ct_set_slots(fhe_ct *ct, int slots);
int fhe_ct_free(fhe_ct *ct);
/* sum_i ct_i * pt_i with ONE rescale: the masked sums of vecRotsOpt /
 * blindRotationOptN (src/sort_algo.h:341-346, 573-577; OpenFHE FLEXIBLEAUTO
 * rescales the sum lazily).  All operands at one level; cts share a batch. */
int fhe_mul_plain_sum(fhe_ctx *ctx, const fhe_ct *const *cts, const fhe_pt *const *pts, int m, fhe_ct **out);
/* The masked sums of `nb` batches over one list of `m` single ciphertexts (the
 * comparator batches of a DirectSort chunk share their baby steps): member b of
 * the result is fhe_mul_plain_sum(cts, pts + b * m, m) word for word, formed by
 * one kernel over every batch and one rescale.  pts: nb * m handles, batch-major.
 * FHE_RANK_STACK_MASKS=0 runs the nb sums and stacks them. */
int fhe_mul_plain_sum_batches(fhe_ctx *ctx, const fhe_ct *const *cts, const fhe_pt *const *pts, int m, int nb,
                              fhe_ct **out);
/* batches a thread of that kernel keeps, and the limbs of n words one pass over
 * nb batches of m terms moves with that tile: 2 m ceil(nb / tile) + m nb + 2 nb
 * (nb (3 m + 2) for nb separate sums); < 0 for a tile < 1 */
int fhe_plain_sum_tile(void);
double fhe_plain_sum_batches_limb_units(int m, int nb, int tile);
/* ciphertext batches: `m` ciphertexts at one level stacked into one handle of
 * batch sum(batch_i) ([batch][2][limbs][n]); every op applies member-wise in
 * the same kernel launches (the reference loops over batches instead:
 * src/sort_algo.h:474-491, 713-742).  member() is a view (no copy);
 * sum_members() adds all members into one ciphertext. */
int fhe_ct_stack(fhe_ctx *ctx, const fhe_ct *const *xs, int m, fhe_ct **out);
int fhe_ct_member(fhe_ctx *ctx, const fhe_ct *a, int m, fhe_ct **out);
int fhe_ct_sum_members(fhe_ctx *ctx, const fhe_ct *a, fhe_ct **out);
/* MakeCKKSPackedPlaintext(v, 1, level, nullptr, slots) (src/sort_algo.h:341,573) */
int fhe_pt_encode(fhe_ctx *ctx, const double *v, int len, int slots, int level, fhe_pt **out);
int fhe_pt_upload(fhe_ctx *ctx, const uint64_t *host, int limbs, int level, int slots, double scale,
                  fhe_pt **out);
int fhe_pt_free(fhe_pt *pt);
/* limbs of a plaintext (< 0 on a null handle), and its words [limbs][n] (NTT form) */
int fhe_pt_limbs(const fhe_pt *pt);
int fhe_pt_download(fhe_ctx *ctx, const fhe_pt *pt, uint64_t *out);
/* the same plaintext as fhe_pt_encode, word for word, encoded on the device
 * (special inverse FFT in fp64 restating the host encoder's operations,
 * rounding, RNS split, NTT: csrc/device/encode.hip) */
int fhe_pt_encode_device(fhe_ctx *ctx, const double *v, int len, int slots, int level, fhe_pt **out);
/* `count` DirectSort masks generated and encoded on the device in one batch:
 * spec[4 i .. 4 i + 3] = {kind, k, r, level}; kind 0 = mask_vector(num_slots,
 * N, k) rotated by r (src/sort_algo.h:206-233, 289-306), kind 1 =
 * checking_vector(num_slots, N, k) (src/sort_algo.h:272-286); each equals
 * fhe_pt_encode of that vector word for word.  out: `count` handles */
int fhe_pt_encode_masks(fhe_ctx *ctx, const int32_t *spec, int count, int num_slots, int N, fhe_pt **out);

/* -------------------------------------------------------------------- ops */
/* EvalAdd / EvalSub (src/comparison.cpp:13,19; src/sort_algo.h:454,495,504) */
int fhe_add(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *b, fhe_ct **out);
int fhe_sub(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *b, fhe_ct **out);
int fhe_negate(fhe_ctx *ctx, const fhe_ct *a, fhe_ct **out);
/* EvalAdd(ct, double) / EvalMult(ct, double) (src/comparison.cpp:19; src/sign.cpp:25-32) */
int fhe_add_const(fhe_ctx *ctx, const fhe_ct *a, double c, fhe_ct **out);
int fhe_mul_const(fhe_ctx *ctx, const fhe_ct *a, double c, fhe_ct **out);
int fhe_mul_const_to(fhe_ctx *ctx, const fhe_ct *a, double c, int target_level, fhe_ct **out);
int fhe_mul_int(fhe_ctx *ctx, const fhe_ct *a, int64_t k, fhe_ct **out);
int fhe_level_adjust(fhe_ctx *ctx, const fhe_ct *a, int target_level, fhe_ct **out);
int fhe_rescale(fhe_ctx *ctx, const fhe_ct *a, fhe_ct **out);
/* EvalMult(ct, pt) (src/sort_algo.h:344,576) / EvalAdd(ct, pt) */
int fhe_mul_plain(fhe_ctx *ctx, const fhe_ct *a, const fhe_pt *p, fhe_ct **out);
int fhe_add_plain(fhe_ctx *ctx, const fhe_ct *a, const fhe_pt *p, fhe_ct **out);
/* EvalMultAndRelinearize / EvalMult(ct,ct) / EvalSquare (src/sign.cpp:23-33; sort_algo.h:730) */
int fhe_mul_relin(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *b, fhe_ct **out);
int fhe_square_relin(fhe_ctx *ctx, const fhe_ct *a, fhe_ct **out);
/* (a [+ a_add]) * b + sum_i c_i x_i [+ raw] with one relinearisation and one rescale (the
   Paterson-Stockmeyer products of fhe_cheb_ps): m summands x_i at levels <= a's, formed at the
   product's pre-rescale scale; raw (or NULL) a ciphertext of a's level added to the tensor as it
   is; a_add (or NULL) a ciphertext of a's level and batch added to a first */
int fhe_mul_add(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *b, const fhe_ct *const *xs, const double *c, int m,
                const fhe_ct *raw, const fhe_ct *a_add, fhe_ct **out);
/* fhe_mul_add with two constants: (a [+ a_add] + a_const) * b + ... + out_const.  a_const is
   at a's scale and added on load in the tensor pass, out_const at the result's scale and added
   there as a term of d0 (times the prime the rescale drops, on the limbs below it): the words
   of fhe_add_const before and after the product (0 = none).
   FHE_MUL_FOLD_CONST=0, or an a below b's level, takes those separate steps instead. */
int fhe_mul_add_const(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *b, const fhe_ct *const *xs, const double *c, int m,
                      const fhe_ct *raw, const fhe_ct *a_add, double a_const, double out_const, fhe_ct **out);
/* whether a_const is folded (1) or formed first (0) for operands at these levels */
int fhe_mul_fold_left(int enabled, int a_level, int b_level);
/* EvalRotate(ct, k) (src/rotation.h:224,231); FHE_ENOKEY if k has no key */
int fhe_rotate(fhe_ctx *ctx, const fhe_ct *a, int k, fhe_ct **out);
/* EvalFastRotationPrecompute + EvalFastRotation (src/rotation.h:281,342-346) */
int fhe_rotate_hoisted(fhe_ctx *ctx, const fhe_ct *a, const int32_t *ks, int m, fhe_ct **outs);
/* EvalLinearWSum-style sum_i c_i x_i rescaled to target_level */
int fhe_linear_sum_to(fhe_ctx *ctx, const fhe_ct *const *xs, const double *c, int m, int target_level,
                      fhe_ct **out);
/* EvalChebyshevSeriesPS(ct, coeffs, a, b) (src/sort_algo.h:629,727; src/sign.cpp:76) */
int fhe_cheb_ps(fhe_ctx *ctx, const fhe_ct *a, const double *coeffs, int ncoeffs, double lo, double hi,
                fhe_ct **out);

/* ---------------------------------------------------- comparator surface */
/* compositeSign<n>(x, cc, SignConfig(CompositeSignConfig(n, dg, df))) (src/sign.cpp:160-185) */
int fhe_sign_composite(fhe_ctx *ctx, const fhe_ct *x, int n, int dg, int df, fhe_ct **out);
/* Comparison::compare(cc, a, b, CompositeSign, cfg) (src/comparison.cpp:4-22) */
int fhe_compare(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *b, int n, int dg, int df, fhe_ct **out);
/* Comparison::indicator(cc, x, c, CompositeSign, cfg) (src/comparison.cpp:24-40) */
int fhe_indicator(fhe_ctx *ctx, const fhe_ct *x, double c, int n, int dg, int df, fhe_ct **out);
/* RotationComposer<N>(cc, enc, rots, algo).rotate(ct, rotation) (src/rotation.h:205-233);
 * algo: 0 NAF, 1 BNAF, 2 BINARY */
int fhe_compose_rotate(fhe_ctx *ctx, const fhe_ct *a, int N, const int32_t *rots, int nrot, int algo,
                       int rotation, fhe_ct **out);
/* Member m of the ciphertext batch `a` rotated by rotations[m] through the same keyed
 * steps as fhe_compose_rotate, step j of every member in one multi-key launch sequence
 * (the batched giant steps of blindRotationOptN / vecRotsOpt, src/sort_algo.h:326-366,
 * 561-584); *out is the batch of the results, word-identical to member-wise rotation. */
int fhe_compose_rotate_members(fhe_ctx *ctx, const fhe_ct *a, int N, const int32_t *rots, int nrot, int algo,
                               const int32_t *rotations, int count, fhe_ct **out);
/* RotationTree<N>(cc, rots, algo) (src/rotation.h:240-358): buildTree(start, end)
 * (:272-279), treeRotate(ct, rotation) (:281-291) with every node's rotation cached
 * (one tree per input ciphertext, as in the reference) and the children of a node
 * sharing one ModUp; getStats() (:168-191) as {fast, normal, total, cache hits,
 * cache misses}.  A rotation whose path was not built returns the partial rotation
 * after a message on stderr, like the reference (:323-327). */
typedef struct fhe_rot_tree fhe_rot_tree;
int fhe_rotation_tree_create(fhe_ctx *ctx, int N, const int32_t *rots, int nrot, int algo, fhe_rot_tree **out);
int fhe_rotation_tree_build(fhe_rot_tree *t, int start, int end);
int fhe_rotation_tree_rotate(fhe_rot_tree *t, const fhe_ct *a, int rotation, fhe_ct **out);
int fhe_rotation_tree_stats(const fhe_rot_tree *t, uint64_t stats[5]);
void fhe_rotation_tree_destroy(fhe_rot_tree *t);
/* Decomposer<N>(rots).decompose(rotation, wrapN, algo) (src/rotation.h:54-102); returns #steps */
int fhe_decompose(int N, const int32_t *rots, int nrot, int rotation, int wrap_n, int algo, int32_t *values,
                  int32_t *sizes, int max_steps);

/* -------------------------------------------------------------- rank sort */
/* DirectSort<N>::getSizeParameters (src/sort_algo.h:87-201); returns #rotations */
int fhe_size_parameters(int N, int *mult_depth, int32_t *rots, int max_rots);
/* u64 sum of `count` device words over all ranks, in place (RCCL, MPI, ...).
 * Called with the context stream drained; the sum must be complete on return.
 * Returns 0 on success; any other value aborts the sort with FHE_EHIP.  Sums
 * are exact while world * q_max < 2^64 (world <= 16 at a 60-bit q0): a larger
 * world is refused with FHE_EINVAL before any work. */
typedef int (*fhe_allreduce_fn)(uint64_t *dev_data, uint64_t count, void *user);
/* DirectSort<N>(cc, pk, rots, enc).{sort | constructRank | rotationIndexCheckN}
 * (src/sort_algo.h:752-774 / 368-506 / 658-750); mode 0 sort, 1 rank, 2 index
 * check (then `rank` is the rank ciphertext).  Batches b with b % world == rank
 * run locally (1 <= shard_world, 0 <= shard_rank < shard_world, else
 * FHE_EINVAL); partial ranks/outputs are summed with `allreduce` when given;
 * else with the RCCL communicator of fhe_comm_init when shard_world equals its
 * world (shard_rank must then be the communicator rank; a world-1 communicator
 * runs its one-rank reduction through RCCL); else shard_world must be 1 and the
 * sort is local -- so an unsharded sort (0, 1) still runs on a context that
 * joined a larger communicator. */
int fhe_direct_sort(fhe_ctx *ctx, const fhe_ct *x, const fhe_ct *rank, int N, const int32_t *rots, int nrot,
                    int n, int dg, int df, int mode, int shard_rank, int shard_world, fhe_allreduce_fn allreduce,
                    void *user, fhe_ct **out);

/* Records sorted by an encrypted key.  out[p] = rotationIndexCheckN(rank(key), cols[p]),
 * word for word what ncols calls of fhe_direct_sort(mode 2) give, with the index
 * series evaluated once.  rank == NULL: constructRank(key) first (key must then be
 * given); rank != NULL: key may be NULL (apply a known rank to the columns).
 * Pass the key among cols to get it sorted too.  Sharding as fhe_direct_sort.
 * FHE_EINVAL (the message names the column) for ncols < 1, a null column, a column
 * that is a stack, a column whose slot count differs from the rank's (or, without a
 * rank, the key's), and for a missing key and rank; FHE_EDEPTH for a column below
 * the level of the series output (the product could not meet it there), raised
 * before the index check starts.  On failure no output handle is set.  With tied
 * keys the columns are mixed exactly as the key is (tests/tie_model.py) unless
 * fhe_set_sort_tiebreak is set: then the rank built here is the stable one and
 * the columns come out in the stable permutation.  A rank passed in is used as
 * given. */
int fhe_direct_sort_columns(fhe_ctx *ctx, const fhe_ct *key, const fhe_ct *rank, const fhe_ct *const *cols,
                            int ncols, int N, const int32_t *rots, int nrot, int n, int dg, int df,
                            int shard_rank, int shard_world, fhe_allreduce_fn allreduce, void *user,
                            fhe_ct **outs /* ncols handles */);
/* most members (columns x stacked batches) of one stacked column product of
 * fhe_direct_sort_columns (default 256, or FHE_SORT_COLS_MEMBERS at context
 * creation; HBM use grows with it); more columns run in groups.  Results do
 * not depend on it. */
int fhe_set_sort_column_members(fhe_ctx *ctx, int max_members);
/* for tests and bindings, like fhe_mul_add: the stack a (B members) times ncols
 * single ciphertexts, member p B + z = fhe_mul_relin(member z, cols[p]) word for
 * word (one tensor pass; FHE_SORT_COLS_FUSED=0: ncols broadcast products,
 * stacked); and out[p] = sum_z a[p B + z] for `groups` groups of consecutive
 * members in one launch (under the same switch: one member sum per group) */
int fhe_mul_columns(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *const *cols, int ncols, fhe_ct **out_stack);
int fhe_ct_sum_member_groups(fhe_ctx *ctx, const fhe_ct *a, int groups, fhe_ct **out_stack);

/* Order statistics by encrypted rank (the project's own extension, like
 * fhe_direct_sort_columns; the reference has no such function).  targets[0 ..
 * ntargets) are ranks in [0, N), in any order, repeats allowed, 1 <= ntargets <=
 * N.  out[c] has N slots: slot p < ntargets holds cols[c]'s value at the element
 * whose rank is targets[p], the other slots hold zero; the level is the sort's
 * output level.  rank == NULL: constructRank(key) first; rank != NULL (what
 * fhe_direct_sort mode 1 returns): key may be NULL.  Pass the key among cols for
 * the k-th smallest key itself.  With num_slots = N P_ slots (the rank's shape)
 * one ciphertext serves P_ - 1 targets (1 when P_ = 1), each on its own window
 * of N slots (fhe_select_layout), so ntargets <= P_ - 1 cost one evaluation of the
 * index series on one ciphertext instead of the sort's N / P_ stacked ones, and any
 * ntargets cost ceil(ntargets / (P_ - 1)); the members run stacked in chunks of
 * fhe_set_sort_stack, and the result does not depend on the chunking.
 * Unsharded: a sharded caller builds the rank with fhe_direct_sort(mode 1,
 * shard ...) and passes it in.  FHE_EINVAL (the message names the column) for
 * ncols < 1, a null column, a column that is a stack, a column whose slot count
 * differs from the rank's (or, without a rank, the key's); FHE_EINVAL for a
 * missing key and rank, for ntargets outside 1..N and for a target outside
 * [0, N) (the message names the first such target's index); FHE_EDEPTH for a
 * column below the level of the series output.  On failure every output handle
 * is NULL.  With tied keys the result mixes values exactly as the sort does
 * (tests/tie_model.py) unless fhe_set_sort_tiebreak is set: then the rank built
 * here is the stable one and the order statistics are exact.  A rank passed in
 * is used as given.  With fhe_set_mask_cache(ctx, 0) a call re-encodes its own
 * plaintexts at its start. */
int fhe_direct_select(fhe_ctx *ctx, const fhe_ct *key, const fhe_ct *rank, const fhe_ct *const *cols, int ncols,
                      const int32_t *targets, int ntargets, int N, const int32_t *rots, int nrot, int n, int dg,
                      int df, fhe_ct **outs /* ncols handles */);
/* pure host: the layout of such a select over num_slots = N P_ slots (N and P_
 * powers of two, P_ <= N).  cap = P_ - 1 (1 when P_ = 1); target p belongs to
 * member[p] = p / cap and owns the cyclic window of N slots from start[p] =
 * ((p % cap) (N + 1) + member[p] cap) mod num_slots on, so start[p] = p mod N and
 * the windows of one member are disjoint.  Writes min(ntargets, max) entries of
 * each array (either may be NULL); returns the member count ceil(ntargets / cap),
 * or -FHE_EINVAL. */
int fhe_select_layout(int N, int num_slots, int ntargets, int32_t *member, int32_t *start, int max);
/* for tests and bindings: the two plaintexts of member `member` of that select,
 * generated and encoded on the device: out[0] (level_c) holds targets[p] on the
 * window of every target p of the member, out[1] (level_k) holds 1 at the first
 * slot of each of its windows, both 0 elsewhere; each equals fhe_pt_encode of
 * that vector word for word. */
int fhe_pt_encode_select(fhe_ctx *ctx, const int32_t *targets, int ntargets, int member, int num_slots, int N,
                         int level_c, int level_k, fhe_pt **out /* 2 handles */);
/* and its pick sums: `stack` holds groups * npts members, group-major; member g
 * of the result is fhe_mul_plain_sum over members g npts .. g npts + npts - 1
 * and pts, word for word, formed by one kernel over every group and one rescale
 * (FHE_SELECT_FUSED=0: one fhe_mul_plain_sum per group, stacked). */
int fhe_mul_plain_sum_groups(fhe_ctx *ctx, const fhe_ct *stack, const fhe_pt *const *pts, int npts, int groups,
                             fhe_ct **out);

/* Tie-breaking for keys that contain equal values (the project's own extension;
 * DESIGN.md §6.3).  The reference's rank gives a value of multiplicity m the rank
 * #{smaller} + (m - 1) / 2, so tied inputs do not sort (tests/tie_model.py).  With
 * eps > 0 every entry that builds a rank -- fhe_direct_sort modes 0 and 1,
 * fhe_direct_sort_columns and fhe_direct_select with rank == NULL, fhe_sort_hybrid
 * mode 0 -- adds a public offset to each difference x_e - x_j before the sign:
 * +eps where j <= e (the self comparison included), -eps where j > e.  The rank
 * is then the stable argsort rank #{x_j < x_e} + #{j < e : x_j = x_e}: among equal
 * values the earlier index comes first.  The offset is a plaintext addition:
 * levels, depth, keys and the output level are the plain sort's, and no sign is
 * evaluated at 0.  The caller guarantees that
 *   - distinct values differ by at least 2 eps,
 *   - the sign configuration (n, dg, df) resolves eps: sign(+-eps) = +-1 to the
 *     precision the index check needs,
 *   - |x_i - x_j| + eps <= 1, the sign's domain.
 * eps = 0 (the default) is the reference's rank, word for word as before.
 * 0 <= eps < 0.5, else FHE_EINVAL.  A rank passed in (mode 2, rank != NULL) is
 * used as given.  The offset plaintexts are cached per context like the masks
 * (fhe_set_mask_cache(ctx, 0): re-encoded at the start of every rank). */
int fhe_set_sort_tiebreak(fhe_ctx *ctx, double eps);
/* Tables of different sizes in the all-pairs operators (the project's own
 * extension).  (0, 0), the default: every call behaves word for
 * word as before, both tables holding N rows in N slots.  With (n_left, n_right)
 * set, fhe_direct_group_sum, fhe_direct_running_sum, fhe_direct_window_sum and
 * fhe_direct_gather pair a left table of n_left rows with a right table of
 * n_right rows: they require N == max(n_left, n_right), the left operands
 * (left_key, left_lo, part_left[], order_left, order_lo, pos_l) with n_left slots,
 * the right operands and every column with n_right slots, and return outputs of
 * n_left slots; rots stay fhe_size_parameters(N)'s and no level is consumed
 * beyond the square call's.  The walk costs min(n_left, n_right) / P' comparator
 * batches (fhe_pair_shape) where the square one costs N / P_.  (N, N) gives the
 * square call's words.  FHE_EINVAL: a count that is no power of two or below 2,
 * max(n_left, n_right) not a size fhe_size_parameters knows or above the ring's
 * n / 2 slots; at call time N != max(n_left, n_right), an operand whose slot count
 * does not fit (the message names the argument and both counts), and
 * FHE_RUN_ROWS / FHE_WIN_ROWS under n_left != n_right.  fhe_direct_sort*,
 * fhe_direct_select and fhe_direct_lex_rank do not read the setting. */
int fhe_set_pair_tables(fhe_ctx *ctx, int n_left, int n_right);
/* pure host: the layout of such a call on a ring of ring_slots = n / 2 slots.
 * With N = max, m = min of the counts and P_ = min(N, ring_slots / N):
 * num_partition = P' = min(P_, m), num_batch = m / P', num_slots = N P', np the
 * baby steps of (N, P'), fold_steps = log2(n_right / n_left) rounds of the
 * residue fold when n_left < n_right, else 0.  Slot s of batch b pairs left row
 * (s mod N) mod n_left with right row (s mod N + t) mod n_right, t = b P' + s / N.
 * n_left == n_right gives the rank's shape.  Any pointer may be NULL.
 * FHE_EINVAL as fhe_set_pair_tables, and for a ring_slots that is no power of
 * two. */
int fhe_pair_shape(int n_left, int n_right, int ring_slots, int *num_partition, int *num_batch, int *num_slots,
                   int *np, int *fold_steps);
/* pure host: the offsets of comparator batch `batch` over num_slots = N P_ slots
 * (N and P_ powers of two, P_ <= N, 0 <= batch < N / P_).  Slot s compares element
 * e = s mod N with element (e + t) mod N, t = batch P_ + s / N; out[s] = +eps where
 * e + t >= N or t == 0, -eps elsewhere.  Writes num_slots doubles. */
int fhe_tiebreak_offsets(int N, int num_slots, int batch, double eps, double *out);
/* for tests and bindings: those vectors of `count` batches, filled and encoded on
 * the device as one batch at `level`; each equals fhe_pt_encode of its vector
 * word for word. */
int fhe_pt_encode_tiebreak(fhe_ctx *ctx, const int32_t *batches, int count, int num_slots, int N, double eps,
                           int level, fhe_pt **out /* count handles */);
/* and the differences they enter: member i of the result is fhe_add_plain(fhe_sub(a,
 * bs[i]), ps[i]) word for word, written into the stack by one kernel that loads a
 * once per four members (FHE_TIEBREAK_FUSED=0, read once per process: the
 * stacked differences, then one c0 addition per member).  The bs share a level;
 * a at a lower level is level-adjusted once, a at a higher one takes per-member
 * operations; the ps sit at the differences' level, else FHE_EINVAL. */
int fhe_sub_add_plain_stacked(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *const *bs, const fhe_pt *const *ps,
                              int count, fhe_ct **out);

/* Group sums and lookups over rows with equal keys (the project's own extension,
 * like fhe_direct_select).  left_key, right_key and every column
 * hold N rows in N slots.  outs[p] has N slots; slot e holds
 *     sum_j [ |left_key_e - right_key_j| < eps ] cols[p]_j,   j = 0 .. N - 1,
 * and *count_out (optional) the same sum without the column: the number of
 * matching right rows.  With right_key = left_key this is SUM(v) OVER (PARTITION
 * BY key) and COUNT(*) per key, the row itself being part of its group; with a
 * second table's key and columns it is the lookup of SELECT b.v FROM a LEFT JOIN b
 * ON a.k = b.k, zero where no right key matches (unique right keys give the
 * matching row's value).  Slot e of every output belongs to left row e.
 * The computation is constructRank's all-pairs comparison with "equal" in place of
 * "smaller": the match indicator of a pair is (sign(d + eps) + sign(-d + eps)) / 2
 * for the difference d, multiplied into the equally shifted column and summed
 * over the right rows.  The caller guarantees the tie-break's conditions:
 *   - equal keys are equal up to noise far below eps,
 *   - distinct keys differ by at least 2 eps,
 *   - |left_key_e - right_key_j| + eps <= 1, the sign's domain,
 *   - the sign configuration (n, dg, df) resolves eps,
 * and 0 < eps < 0.5.  Levels (fhe_group_sum_levels): with the keys at level k and
 * the sign consuming D levels, the differences sit at k + 1, the indicator at
 * L_m = k + 1 + D, a column may sit at col_max_level = L_m - 2 at most (it is
 * halved on its way to L_m - 1 and meets the indicator after one masked sum), and
 * every output ends at out_level = L_m + 1, where fhe_direct_sort mode 1 ends: the
 * depth of any context built for the sort suffices.  rots are the sort's rotation
 * keys (fhe_size_parameters(N)).  The batches run stacked in chunks of
 * fhe_set_sort_stack on fhe_set_sort_lanes lanes, the columns in groups bounded by
 * fhe_set_sort_column_members; the result does not depend on any of them, nor on
 * fhe_set_mask_cache (0: the call re-encodes the cached masks at its start).
 * Unsharded.  fhe_set_sort_tiebreak has no effect here.
 * FHE_EINVAL (the message names the column where one is at fault) for a null key,
 * a key or column that is a stack, slot counts that differ, keys at different
 * levels, eps outside (0, 0.5), ncols < 0, a null column, and ncols == 0 without
 * count_out; FHE_EDEPTH, before any work, for a column above col_max_level and
 * for a context without out_level levels.  On failure no output handle is set
 * (every one is NULL).
 * Tables of different sizes (fhe_set_pair_tables(ctx, Nl, Nr), N = max(Nl, Nr)):
 * left_key has Nl slots, right_key and every column Nr, the outputs Nl, at
 * min(Nl, Nr) / P' comparator batches (fhe_pair_shape) instead of N / P_ and at
 * the same levels.  GROUP BY over a known domain is the call with the domain's
 * values as left_key.
 * Tables whose row count is no power of two are padded to one: sentinel keys at
 * least 2 eps from every real key and zero columns; such rows match nothing and
 * add nothing, to the counts either. */
int fhe_direct_group_sum(fhe_ctx *ctx, const fhe_ct *left_key, const fhe_ct *right_key, const fhe_ct *const *cols,
                         int ncols, double eps, int N, const int32_t *rots, int nrot, int n, int dg, int df,
                         fhe_ct **outs /* ncols handles */, fhe_ct **count_out /* may be NULL */);
/* pure host: the levels above for keys at key_level under the composite sign
 * (n, dg, df), n = 3 or 4 (g_4's series depth taken under the default
 * Paterson-Stockmeyer split).  Either pointer may be NULL.  FHE_EINVAL for a
 * negative level or degree or another n. */
int fhe_group_sum_levels(int key_level, int n, int dg, int df, int *col_max_level, int *out_level);
/* for tests and bindings: the two-sided differences, member i of the 2 count
 * stack = fhe_add_const(fhe_sub(a, bs[i]), c) and member count + i =
 * fhe_add_const(fhe_negate(fhe_sub(a, bs[i])), c) word for word, written by one
 * kernel from one load of each bs[i], a loaded once per four members
 * (FHE_GROUP_FUSED=0, read once per process: the stacked differences, then
 * negate / add_const on the stack).  The bs share a level; a at a lower level is
 * level-adjusted once, a at a higher one takes per-member operations. */
int fhe_sub_pm_const_stacked(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *const *bs, int count, double c,
                             fhe_ct **out);
/* and the products they feed: a and a_add are stacks of B members, b_stack a
 * column-major stack of ncols B members, all at one level; member p B + z of the
 * result = fhe_mul_relin(fhe_add(member z of a, member z of a_add), member p B + z
 * of b_stack) word for word (one tensor pass that forms a + a_add once per four
 * columns; FHE_GROUP_FUSED=0: ncols fhe_mul_add products with a_add, stacked).
 * FHE_EINVAL for member counts or levels that do not fit. */
int fhe_mul_pairs(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *a_add, const fhe_ct *b_stack, int ncols,
                  fhe_ct **out_stack);

/* Gather by encrypted position: LAG / LEAD and lookups by rank or index (the
 * project's own extension).  pos_l and pos_r are single ciphertexts
 * of N slots at one level holding integers in [0, N) up to the noise a rank
 * carries, the right positions distinct; cols are ncols >= 0 single ciphertexts of
 * N slots, offsets noffsets >= 1 public integers with |o| <= N - 1.  For column p
 * and offset k the output holds at slot e
 *     sum_j delta(pos_l_e + offsets[k] - pos_r_j) cols[p]_j,   j = 0 .. N - 1:
 * the value of the right row standing offsets[k] places after left row e's
 * position, zero where there is none (SQL's NULL, given as 0).  With pos_l = pos_r
 * = a rank (fhe_direct_sort mode 1; with tied keys one built under
 * fhe_set_sort_tiebreak) offset -k is LAG(v, k) and +k LEAD(v, k) in key order; with
 * pos_r an encrypted 0 .. N - 1 and pos_l encrypted indices it is cols[p][idx].
 * want_present != 0 appends per offset the same sum without the column: 1 where the
 * neighbour exists.  sum_offsets != 0 adds the offsets' indicators before the
 * product: one output per column, the sum over the offsets (a ROWS BETWEEN frame),
 * and one present output, the frame's row count.  outs receives, in this order, the
 * gathered columns column-major (index p K + k, K = noffsets, or p alone under
 * sum_offsets), then the present outputs: (ncols + (want_present != 0)) * K handles.
 * The computation is constructRank's all-pairs layout with the index check's
 * predicate: the sort's doubled-sinc series of (pos_l_e + o - pos_r_j) / 2N, the
 * difference negated for o < 0 so that it stays above -N, multiplied into the
 * equally shifted column and summed over the right rows.  Levels
 * (fhe_gather_levels): with the positions at level k the differences sit at k + 1,
 * the series output and the present outputs at series_level, a column may sit at
 * col_max_level = series_level - 2 at most, and the gathered columns end at
 * out_level = series_level + 1; a rank from a level-0 key ends inside
 * fhe_size_parameters(N)'s depth.  rots are the sort's rotation keys.  The batches
 * run stacked in chunks of fhe_set_sort_stack / K on fhe_set_sort_lanes lanes, the
 * columns in groups bounded by fhe_set_sort_column_members; the result does not
 * depend on any of them, nor on fhe_set_mask_cache.  Unsharded.
 * fhe_set_sort_tiebreak has no effect here.
 * FHE_EINVAL (the message names the column or offset at fault) for a null
 * position, a position or column that is a stack, slot counts that differ,
 * positions at different levels, ncols < 0, a null column, noffsets < 1, an offset
 * outside [-(N - 1), N - 1], and ncols == 0 without want_present; FHE_EDEPTH, before
 * any work, for a column above col_max_level and for a context without the
 * levels.  On failure no output handle is set (every one is NULL).
 * Tables of different sizes (fhe_set_pair_tables(ctx, Nl, Nr), N = max(Nl, Nr)):
 * pos_l has Nl slots, pos_r and every column Nr, the outputs Nl; positions,
 * offsets and the series' table stay those of N, so fhe_gather_levels(.., N)
 * holds.  Nl queries into a table of Nr rows cost min(Nl, Nr) / P' batches
 * (fhe_pair_shape).
 * Tables whose row count is no power of two are padded to one: sentinel
 * positions no real position plus an offset reaches (right rows) or that reach
 * no right row (left rows) and zero columns; such rows match nothing and add
 * nothing, to the present flags either. */
int fhe_direct_gather(fhe_ctx *ctx, const fhe_ct *pos_l, const fhe_ct *pos_r, const fhe_ct *const *cols, int ncols,
                      const int32_t *offsets, int noffsets, int want_present, int sum_offsets, int N,
                      const int32_t *rots, int nrot, fhe_ct **outs);
/* pure host: the levels above for positions at pos_level over N rows (the series'
 * depth taken under the default Paterson-Stockmeyer split).  Any pointer may be
 * NULL.  FHE_EINVAL for a negative level or N < 1. */
int fhe_gather_levels(int pos_level, int N, int *col_max_level, int *series_level, int *out_level);
/* for tests and bindings: the oriented, offset differences, member k count + i of
 * the noffsets count stack = fhe_add_const(fhe_sub(a, bs[i]), offsets[k]), negated
 * (fhe_negate) for offsets[k] < 0, word for word, written by one kernel from one
 * load of each bs[i], a loaded once per four members (FHE_GATHER_FUSED=0, read
 * once per process: the stacked differences, then add_const / negate on the stack
 * per offset).  The bs share a level; a at a lower level is level-adjusted once, a
 * at a higher one takes per-member operations. */
int fhe_sub_offsets_stacked(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *const *bs, int count, const int32_t *offsets,
                            int noffsets, fhe_ct **out);
/* and the products they feed: a_stack holds noffsets B members (member k B + z),
 * b_stack ncols B members column-major, all at one level; member (p noffsets + k) B
 * + z of the result = fhe_mul_relin(member k B + z of a_stack, member p B + z of
 * b_stack) word for word (one tensor pass that loads a column's words once per four
 * offsets; FHE_GATHER_FUSED=0: one stacked product per column and offset).
 * FHE_EINVAL for member counts or levels that do not fit. */
int fhe_mul_gather(fhe_ctx *ctx, const fhe_ct *a_stack, const fhe_ct *b_stack, int ncols, int noffsets,
                   fhe_ct **out_stack);

/* Running sums: add up columns over the right rows whose key is smaller than, or
 * within a range of, the left row's (the project's own extension, like
 * fhe_direct_select and fhe_direct_group_sum).  left_key,
 * right_key, left_lo and every column hold N rows in N slots.  outs[p] has N
 * slots; slot e holds
 *     sum_j c_ej cols[p]_j,   j = 0 .. N - 1,
 * and *count_out (optional) sum_j c_ej.  The weight c_ej of a pair by mode, with
 * kl = left_key, kr = right_key:
 *   FHE_RUN_ROWS     (sign(kl_e - kr_j + E_ej) + 1) / 2, E the tie-break offset of
 *                    fhe_set_sort_tiebreak built from this call's eps (+eps where
 *                    j <= e, -eps where j > e): with right_key = left_key the rows
 *                    before row e in the stable order and the row itself, SUM(v)
 *                    OVER (ORDER BY key ROWS UNBOUNDED PRECEDING);
 *   FHE_RUN_LE       (sign(kl_e - kr_j + eps) + 1) / 2: kr_j <= kl_e, peers included --
 *                    SQL's default RANGE frame, SELECT SUM(b.v) FROM b WHERE b.k <= a.k
 *                    per row of a, and with the count searchsorted(side = right);
 *   FHE_RUN_LT       (sign(kl_e - kr_j - eps) + 1) / 2: kr_j < kl_e, searchsorted(side =
 *                    left);
 *   FHE_RUN_BETWEEN  (sign(hi_e - kr_j + eps) - sign(lo_e - kr_j - eps)) / 2 with hi =
 *                    left_key and lo = left_lo: lo_e <= kr_j <= hi_e, both ends closed --
 *                    the band join and RANGE BETWEEN w PRECEDING AND w FOLLOWING.
 * left_lo is required for FHE_RUN_BETWEEN and must be NULL otherwise.  Open ends
 * and descending order are the caller's fhe_add_const / fhe_negate on the keys.
 * The caller guarantees: 0 < eps < 0.5; equal keys agree far below eps; distinct
 * keys, bounds included, differ by at least 2 eps; every sign argument has
 * magnitude <= 1; the sign configuration (n, dg, df) resolves eps; lo_e <= hi_e.
 * The count is halved batch by batch as the rank's compare is, so in FHE_RUN_ROWS
 * with right_key = left_key fhe_add_const(count, -1) is word for word the rank of
 * fhe_direct_sort mode 1 under fhe_set_sort_tiebreak(eps).  Levels are
 * fhe_group_sum_levels': a column may sit at col_max_level at most and every
 * output ends at out_level.  The batches run stacked in chunks of
 * fhe_set_sort_stack on fhe_set_sort_lanes lanes, the columns in groups bounded by
 * fhe_set_sort_column_members; the result does not depend on any of them, nor on
 * fhe_set_mask_cache (0: the call re-encodes the cached masks at its start).
 * Unsharded.  fhe_set_sort_tiebreak has no effect here.  FHE_RUN_FUSED=0, read
 * once per process, takes the unfused forms of the two entries below; same words.
 * FHE_EINVAL for everything fhe_direct_group_sum refuses so, a mode outside 0..3,
 * left_lo given outside FHE_RUN_BETWEEN or missing in it, and a left_lo that is a
 * stack or differs from left_key in level or slot count; FHE_EDEPTH, before any
 * work, for a column above col_max_level and for a context without out_level
 * levels.  On failure no output handle is set (every one is NULL).
 * Tables of different sizes (fhe_set_pair_tables(ctx, Nl, Nr), N = max(Nl, Nr)):
 * left_key and left_lo have Nl slots, right_key and every column Nr, the outputs
 * Nl, at min(Nl, Nr) / P' comparator batches (fhe_pair_shape) and the same
 * levels: Nl query keys searched in Nr sorted keys, the band join.  FHE_RUN_ROWS
 * is FHE_EINVAL under Nl != Nr: its tie-break by index has no meaning between
 * tables of different length.
 * Tables whose row count is no power of two are padded to one: sentinel keys at
 * least 2 eps from every real key and bound and zero columns; such rows match nothing and
 * add nothing, to the counts either. */
#define FHE_RUN_ROWS 0
#define FHE_RUN_LE 1
#define FHE_RUN_LT 2
#define FHE_RUN_BETWEEN 3
int fhe_direct_running_sum(fhe_ctx *ctx, const fhe_ct *left_key, const fhe_ct *left_lo /* NULL unless BETWEEN */,
                           const fhe_ct *right_key, const fhe_ct *const *cols, int ncols, int mode, double eps, int N,
                           const int32_t *rots, int nrot, int n, int dg, int df, fhe_ct **outs /* ncols handles */,
                           fhe_ct **count_out /* may be NULL */);
/* for tests and bindings: the bounded differences, member v count + i of the
 * nbounds count stack = fhe_add_const(fhe_sub(as[v], bs[i]), consts[v]) word for
 * word, nbounds = 1 or 2, written by one kernel that loads each bs[i] once for all
 * bounds and the as once per four members (FHE_RUN_FUSED=0: the stacked
 * differences per bound, then the constant in place).  The as share a level and
 * so do the bs; as at a lower level are level-adjusted once, at a higher one every
 * member takes its own operations. */
int fhe_sub_bounds_stacked(fhe_ctx *ctx, const fhe_ct *const *as, int nbounds, const fhe_ct *const *bs, int count,
                           const double *consts /* nbounds */, fhe_ct **out);
/* and the products they feed: a (and a_sub) are stacks of B members, b_stack a
 * column-major stack of ncols B members, all at one level; member p B + z of the
 * result = fhe_mul_relin(fhe_add_const(member z of a, c), member p B + z of b_stack),
 * resp. fhe_mul_relin(fhe_sub(member z of a, member z of a_sub), ...), word for word
 * (one tensor pass that forms the left operand once per four columns and never
 * writes it; FHE_RUN_FUSED=0: the left operand written out, then ncols products).
 * FHE_EINVAL for member counts or levels that do not fit and ncols < 1. */
int fhe_mul_pairs_const(fhe_ctx *ctx, const fhe_ct *a, double c, const fhe_ct *b_stack, int ncols,
                        fhe_ct **out_stack);
int fhe_mul_pairs_sub(fhe_ctx *ctx, const fhe_ct *a, const fhe_ct *a_sub, const fhe_ct *b_stack, int ncols,
                      fhe_ct **out_stack);

/* Lexicographic rank: order rows by several encrypted key columns (the project's
 * own extension, like fhe_direct_select and fhe_direct_group_sum).
 * keys[0] .. keys[nkeys - 1], most significant first, 2 <= nkeys <= 4, each a single
 * ciphertext of N rows in N slots, all at one level k.  *rank holds at slot e the
 * position of row e among the rows ordered by keys[0], then keys[1], ...: ORDER BY
 * a, b -- or one key wider than the sign resolves, split into digits.  It is an
 * ordinary rank ciphertext and feeds fhe_direct_sort mode 2, fhe_direct_sort_columns
 * and fhe_direct_select (rank != NULL) unchanged.
 * Per pair (e, j) with d_l = keys[l]_e - keys[l]_j:  u_l = sign(d_l + eps) and
 * w_l = sign(d_l - eps) on the leading keys (two signs per leading key, none taken
 * at 0), s = sign(d_last + E) on the last key, E the fhe_set_sort_tiebreak offset
 * when one is set;  T_last = s + 1,  T_l = (u_l - w_l) T_{l+1} + 2^(nkeys-1-l) (w_l + 1),
 * rank_e = 2^-nkeys sum_j T_0 - c.  With the tie-break set c = 1 and the rank is the
 * stable lexicographic argsort rank; without it c = 1/2 and rows tied on every key
 * share their ranks as the plain rank's ties do (tests/tie_model.py).
 * The caller guarantees, as for the group sums:
 *   - values equal on a leading key are equal up to noise far below eps,
 *   - distinct ones differ by at least 2 eps,
 *   - |d_l| + eps <= 1, the sign's domain,
 *   - the sign configuration (n, dg, df) resolves eps,
 *   - the tie-break's own conditions hold on the last key,
 * and 0 < eps < 0.5.  Levels (fhe_lex_rank_levels): with the sign consuming D
 * levels every sign output sits at L_m = k + 1 + D and the rank ends at
 * rank_level = L_m + nkeys, nkeys - 1 levels below where fhe_direct_sort mode 1
 * ends: a context for the lexicographic rank and the index check needs the depth
 * of fhe_size_parameters(N) plus nkeys - 1.  rots are the sort's rotation keys.
 * The batches run stacked in chunks of fhe_set_sort_stack / (2 nkeys - 1) on
 * fhe_set_sort_lanes lanes; the result depends on neither, nor on
 * fhe_set_mask_cache (0: the call re-encodes at its start what it caches).
 * Unsharded: a sharded caller has no use for it yet (the rank it feeds to a
 * sharded index check is computed once and passed in).
 * FHE_EINVAL (the message names the key at fault) for nkeys outside 2..4, a null
 * key, a key that is a stack, slot counts or levels that differ, and eps outside
 * (0, 0.5); FHE_EDEPTH, before any work, for a context without rank_level levels.
 * On failure *rank is NULL. */
int fhe_direct_lex_rank(fhe_ctx *ctx, const fhe_ct *const *keys, int nkeys, double eps, int N, const int32_t *rots,
                        int nrot, int n, int dg, int df, fhe_ct **rank);
/* pure host: rank_level above for nkeys keys at key_level under the composite sign
 * (n, dg, df), n = 3 or 4.  The pointer may be NULL.  FHE_EINVAL for nkeys outside
 * 2..4, a negative level or degree, or another n. */
int fhe_lex_rank_levels(int key_level, int nkeys, int n, int dg, int df, int *rank_level);
/* for tests and bindings: the differences of nkeys keys against count shifted
 * copies each (bs key-major: bs[l count + i]) as one stack of (2 nkeys - 1) count
 * members.  For a leading key l, member (2 l) count + i = fhe_add_const(fhe_sub(as[l],
 * bs[l count + i]), +eps) and member (2 l + 1) count + i the same with -eps; for the
 * last key, member 2 (nkeys - 1) count + i = fhe_sub(as[nkeys - 1], bs[..]), with
 * fhe_add_plain(., ps[i]) when ps is not NULL (count plaintexts at the differences'
 * level); word for word, written by one kernel that loads every b once and a key
 * once per four operands (FHE_LEX_FUSED=0, read once per process: the stacked
 * differences and add_const per key).  The as share a level and so do the bs; as at
 * a lower level are level-adjusted once, at a higher one every member takes its
 * own operations.  FHE_EINVAL for counts or levels that do not fit. */
int fhe_sub_lex_stacked(fhe_ctx *ctx, const fhe_ct *const *as, int nkeys, const fhe_ct *const *bs, int count,
                        const fhe_pt *const *ps /* may be NULL */, double eps, fhe_ct **out);
/* and the Horner step they feed: t, u and w are stacks of B members, u and w at one
 * level; member z of the result = fhe_mul_relin(fhe_add_const(t_z, t_const),
 * fhe_sub(u_z, w_z)) word for word.  With t at the level of u and w it is one tensor
 * pass that adds the constant to c0 as it loads t and forms u - w as it loads them,
 * then the product's relinearisation and rescale; with t at another level, or under
 * FHE_LEX_FUSED=0, the difference is formed first and the product follows.
 * FHE_EINVAL for member counts or levels of u and w that do not fit. */
int fhe_mul_lex(fhe_ctx *ctx, const fhe_ct *t, double t_const, const fhe_ct *u, const fhe_ct *w, fhe_ct **out);

/* Window sums: add up columns over the right rows that agree with the left row on
 * every partition key and that an order key selects (the project's own extension,
 * like fhe_direct_select and the sums before it).  Every key and
 * column holds N rows in N slots; all keys sit at one level.  With nparts
 * partition keys (1..3), part_left[g] the left table's and part_right[g] the right
 * table's (the same handle for a self join), outs[p] holds at slot e
 *     sum_j c_ej cols[p]_j,   c_ej = prod_g [part_left[g]_e = part_right[g]_j] * r_ej,
 * and *count_out (optional) sum_j c_ej.  A partition indicator is
 * (sign(d + eps) - sign(d - eps)) / 2 for d = part_left[g]_e - part_right[g]_j; r_ej is
 * fhe_direct_running_sum's weight for the mode on (order_left, order_lo,
 * order_right) -- FHE_WIN_ROWS / LE / LT / BETWEEN have FHE_RUN_*'s values and
 * meanings -- or 1 under FHE_WIN_GROUP, which takes no order key (every order_*
 * NULL).  With F = nparts + (mode != FHE_WIN_GROUP) factors, 2 <= F <= 4; one
 * partition key under FHE_WIN_GROUP is fhe_direct_group_sum and is refused.
 *   SUM(v) OVER (PARTITION BY g ORDER BY t ROWS UNBOUNDED PRECEDING): nparts = 1,
 *     FHE_WIN_ROWS, self join; its count is ROW_NUMBER(), LE's / LT's count + 1 RANK();
 *   GROUP BY a, b and JOIN ON a.k1 = b.k1 AND a.k2 = b.k2: nparts = 2, FHE_WIN_GROUP;
 *   the as-of join ON a.id = b.id AND b.t <= a.t: nparts = 1, FHE_WIN_LE;
 *   PARTITION BY g ORDER BY t RANGE BETWEEN w PRECEDING AND w FOLLOWING: FHE_WIN_BETWEEN
 *     with order_left = t + w and order_lo = t - w.
 * The caller guarantees fhe_direct_running_sum's conditions on every key: 0 < eps <
 * 0.5; equal values agree far below eps; distinct values, bounds included, differ
 * by at least 2 eps; every sign argument has magnitude <= 1, for pairs of rows from
 * different partitions too; the sign configuration resolves eps.  Levels
 * (fhe_window_sum_levels): the sign outputs sit at L_m = key level + 1 + sign depth,
 * their product after ceil(log2 F) levels at L_a; a column may sit at col_max_level
 * = L_a - 2 at most and every output ends at out_level = L_a + 1.  The batches run
 * stacked in chunks of fhe_set_sort_stack / (2 nparts + V) (V = 0, 1 or 2 sign
 * members for the order key) on fhe_set_sort_lanes lanes, the columns in groups
 * bounded by fhe_set_sort_column_members; the result does not depend on any of
 * them, nor on fhe_set_mask_cache.  Unsharded.  fhe_set_sort_tiebreak has no effect
 * here.  FHE_WIN_FUSED=0, read once per process, takes the unfused forms of the
 * two entries below; same words.  FHE_EINVAL for nparts outside 1..3, F outside
 * 2..4, a mode outside 0..4, an order key under FHE_WIN_GROUP or a missing one
 * otherwise, order_lo outside FHE_WIN_BETWEEN or missing in it, a null handle, a
 * stack, keys at different levels or with a slot count other than N, a column with
 * another slot count, ncols < 0, nothing asked for, and eps outside (0, 0.5);
 * FHE_EDEPTH, before any work, for a column above col_max_level and for a context
 * without out_level levels.  On failure no output handle is set (every one is NULL).
 * Tables of different sizes (fhe_set_pair_tables(ctx, Nl, Nr), N = max(Nl, Nr)):
 * part_left[], order_left and order_lo have Nl slots, part_right[], order_right and
 * every column Nr, the outputs Nl, at min(Nl, Nr) / P' comparator batches
 * (fhe_pair_shape) and the same levels: the as-of join of a small table against
 * a large one, GROUP BY a, b as one row per group.  FHE_WIN_ROWS is FHE_EINVAL
 * under Nl != Nr.
 * Tables whose row count is no power of two are padded to one: sentinel partition keys at
 * least 2 eps from every real key and zero columns; such rows match nothing and
 * add nothing, to the counts either. */
#define FHE_WIN_ROWS 0
#define FHE_WIN_LE 1
#define FHE_WIN_LT 2
#define FHE_WIN_BETWEEN 3
#define FHE_WIN_GROUP 4
int fhe_direct_window_sum(fhe_ctx *ctx, const fhe_ct *const *part_left, const fhe_ct *const *part_right, int nparts,
                          const fhe_ct *order_left /* NULL under GROUP */, const fhe_ct *order_lo /* BETWEEN only */,
                          const fhe_ct *order_right /* NULL under GROUP */, const fhe_ct *const *cols, int ncols,
                          int mode, double eps, int N, const int32_t *rots, int nrot, int n, int dg, int df,
                          fhe_ct **outs /* ncols handles */, fhe_ct **count_out /* may be NULL */);
/* pure host: col_max_level and out_level above for keys at key_level and nfactors
 * factors (2..4) under the composite sign (n, dg, df), n = 3 or 4.  Either pointer
 * may be NULL.  FHE_EINVAL for nfactors outside 2..4, a negative level or degree, or
 * another n. */
int fhe_window_sum_levels(int key_level, int nfactors, int n, int dg, int df, int *col_max_level, int *out_level);
/* for tests and bindings: the sign arguments of nparts partition keys (1..3) against
 * count shifted copies each (part_bs key-major: part_bs[g count + i]) and, unless mode
 * is FHE_WIN_GROUP, of an order key against order_bs (count of them), as one stack.
 * Members (2 g) count + i and (2 g + 1) count + i = fhe_add_const(fhe_sub(part_as[g],
 * part_bs[g count + i]), +eps resp. -eps).  Behind them, from member 2 nparts count on:
 * FHE_WIN_ROWS count members fhe_add_plain(fhe_sub(order_a, order_bs[i]), ps[i]);
 * FHE_WIN_LE / LT count members fhe_add_const(fhe_sub(order_a, order_bs[i]), +eps /
 * -eps); FHE_WIN_BETWEEN count members fhe_add_const(fhe_sub(order_a, order_bs[i]), +eps),
 * then count members fhe_add_const(fhe_sub(order_lo, order_bs[i]), -eps).  Word for
 * word, written by one kernel that loads every operand once and a left operand once
 * per four members (FHE_WIN_FUSED=0, read once per process: the stacked differences
 * per side, then the constant in place or the plaintext per member).  Every left
 * operand shares one level and so do the right ones; left operands at a lower level
 * are level-adjusted once, at a higher one every member takes its own operations.
 * order_lo goes with FHE_WIN_BETWEEN alone, ps (count plaintexts at the differences'
 * level) with FHE_WIN_ROWS alone.  FHE_EINVAL for counts, modes or levels that do
 * not fit. */
int fhe_sub_window_stacked(fhe_ctx *ctx, const fhe_ct *const *part_as, int nparts, const fhe_ct *const *part_bs,
                           int count, int mode, const fhe_ct *order_a, const fhe_ct *order_lo,
                           const fhe_ct *const *order_bs, const fhe_pt *const *ps, double eps, fhe_ct **out);
/* and the product of two indicators: u, w, u2 and w2 are stacks of B members, u and w
 * at one level, u2 and w2 at one level; member z of the result =
 * fhe_mul_relin(fhe_sub(u_z, w_z), fhe_sub(u2_z, w2_z)) word for word.  With all four at
 * one level it is one tensor pass that forms both differences as it loads them and
 * writes neither, then the product's relinearisation and rescale; with the pairs at
 * two levels, or under FHE_WIN_FUSED=0, the differences are formed first and the
 * product follows.  FHE_EINVAL for member counts or levels that do not fit. */
int fhe_mul_sub_sub(fhe_ctx *ctx, const fhe_ct *u, const fhe_ct *w, const fhe_ct *u2, const fhe_ct *w2, fhe_ct **out);

/* how many of a rank's sort batches run stacked through one compare / one
 * sinc PS (default 32: every launch then carries up to 32 ciphertexts; HBM use
 * grows with it).  Results do not depend on it. */
int fhe_set_sort_stack(fhe_ctx *ctx, int max_stack);
/* concurrent lanes per sort (default 2): the rank's batches are split over
 * host threads driving forked engines (own HIP stream and pool, shared keys),
 * so independent batch stacks overlap on the GPU.  Results do not depend on it. */
int fhe_set_sort_lanes(fhe_ctx *ctx, int lanes);

/* Paterson-Stockmeyer split of every Chebyshev series the context evaluates
 * (fhe_cheb_ps, the doubled-sinc index check, g_4, the hybrid sort's sinc,
 * EvalMod).  FHE_PS_SPLIT_OPENFHE (the default) is OpenFHE's
 * EvalChebyshevSeriesPS, which the reference calls (src/sort_algo.h:629,727,
 * src/sign.cpp:76): ComputeDegreesPS's (k, m), long division by T_{k 2^(m-1)},
 * the series padded by a monic T_{k(2^m-1)}.  FHE_PS_SPLIT_ENGINE is rounds 1-2's
 * power-of-two split.  Same polynomial, same depth for the reference's degrees;
 * the OpenFHE split keeps a degree-6510 series within the reference's 0.01 at
 * 40-bit scaling where the other does not. */
#define FHE_PS_SPLIT_ENGINE 0
#define FHE_PS_SPLIT_OPENFHE 1
int fhe_set_ps_split(fhe_ctx *ctx, int split);
int fhe_get_ps_split(const fhe_ctx *ctx);
/* levels a degree-`degree` series consumes under `split` (the output level of
 * fhe_cheb_ps is the input level plus this); < 0 on bad arguments */
int fhe_cheb_ps_depth(int degree, int split);
/* 1 if fhe_cheb_ps under FHE_PS_SPLIT_OPENFHE evaluates these coefficients
 * with OpenFHE's division tree, 0 if it falls back to the power-of-two split
 * (degree < 5, or a quotient coefficient above 1024: DESIGN.md §3); < 0 on bad
 * arguments.  Host only. */
int fhe_cheb_ps_plan(const double *coeffs, int ncoeffs);

/* ------------------------------------------------------------ hybrid sort */
/* DirectSort<N>::sort_hybrid (src/sort_algo.h:1050-1064; mode 0) or
 * rotationIndexCheckHybrid(rank, x) (:893-1047; mode 1): constructRank, then the
 * MEHP24-style matrix index check.  max_array = maxArraySize (the reference's 256;
 * smaller values exercise the multi-block path on small rings: max_array^2 must
 * equal the slot count when N > max_array); mask_mode 0 = the reference's choice
 * by N (scaled-sinc PS below 256, Comparison::indicator with (3,4,2) below 512,
 * (3,5,2) above), 1/2/3 force one of them.  Blocks shard over ranks like
 * fhe_direct_sort (one all-reduce of the partial outputs). */
int fhe_sort_hybrid(fhe_ctx *ctx, const fhe_ct *x, const fhe_ct *rank, int N, const int32_t *rots, int nrot, int n,
                    int dg, int df, int mode, int max_array, int mask_mode, int shard_rank, int shard_world,
                    fhe_allreduce_fn allreduce, void *user, fhe_ct **out);
/* the hybrid test's depth and rotation list (tests/DirectSortHTest.cpp:23-104,
 * ring 2^17); returns #rotations */
int fhe_hybrid_parameters(int N, int *mult_depth, int32_t *rots, int max_rots);

/* ------------------------------------------------------------ MEHP24 sort */
/* the reference's MEHP24 test parameters for N (tests/mehp24/Mehp24SortTest.cpp:26-128)
 * and mehp24::utils::getRotationIndices(N) (src/mehp24/mehp24_utils.cpp:197-225):
 * depth, ring log, scale bits, key-switch digits (dnum: 3, OpenFHE's default),
 * CompositeSign (n, dg, df), indicator (dg_i, df_i), part length (0: one-ciphertext
 * sortFG).  The context gets mult_depth + 1 levels and the input is encrypted with
 * fhe_encrypt_ext (OpenFHE's default FLEXIBLEAUTOEXT).  Returns #rotations. */
int fhe_mehp24_parameters(int N, int *mult_depth, int *log_ring, int *scale_bits, int *dnum, int cfg[3],
                          int *dg_i, int *df_i, int *sub_length, int32_t *rots, int max_rots);
/* getRotationIndices with part length `sub` (the reference fixes 256) */
int fhe_mehp24_rotation_indices(int N, int sub, int32_t *rots, int max_rots);
/* sub == 0: mehp24::sortFG(c, N, CompositeSign, cfg, comp, dg_i, df_i, cc)
 *           (src/mehp24/mehp24_sort.cpp:248-283), x holds N values in N*N slots;
 * sub > 0:  mehp24::sortLargeArrayFG(c, N, sub, ...) (mehp24_sort.cpp:623-645),
 *           x holds N values in sub*sub slots.
 * Independent compares / indicators run stacked (fhe_set_sort_stack bounds it). */
int fhe_mehp24_sort(fhe_ctx *ctx, const fhe_ct *x, int N, int sub, int n, int dg, int df, int dg_i, int df_i,
                    fhe_ct **out);
/* fhe_mehp24_sort with sortLargeArrayFG's P(P+1)/2 pair compares
 * (mehp24_sort.cpp:477-514, an OpenMP loop in the reference) and P^2 indicators
 * (:574-594) sharded over ranks (item i on rank i % shard_world); the partial
 * Cv / Ch / subSorted sums are combined by `allreduce` (or RCCL after
 * fhe_comm_init when it is NULL), so every rank returns the same, unsharded
 * result.  sub == 0 (one ciphertext) has nothing to shard and runs replicated. */
int fhe_mehp24_sort_sharded(fhe_ctx *ctx, const fhe_ct *x, int N, int sub, int n, int dg, int df, int dg_i,
                            int df_i, int shard_rank, int shard_world, fhe_allreduce_fn allreduce, void *user,
                            fhe_ct **out);
/* mehp24::utils::indicatorAdv(c, b, dg, df) (src/mehp24/mehp24_utils.cpp:166-174) */
int fhe_mehp24_indicator(fhe_ctx *ctx, const fhe_ct *x, double b, int dg, int df, fhe_ct **out);

/* ------------------------------------------------ k-way sorting network */
/* kwaySort::Sorter::sorter (src/k-way/Sorter.cpp:289-404) as called by
 * KWayAdapter<N>::sort (src/kway_adapter.h:65-71): sorts the N = k^M values in
 * the first slots of x (k in {2, 3, 5}; x holds next_pow2(N) slots), comparator
 * CompositeSign(3, dg, df) (the reference tests' CompositeSignConfig(3, d_f, d_g)
 * order: tests/k-way/KWaySort2Test.cpp:149).  Without a bootstrapper the
 * context must hold every level (no EvalBootstrap at EvalUtils::
 * checkLevelAndBoot, src/k-way/EvalUtils.cpp:59-86), otherwise FHE_EDEPTH.
 * Rotation keys: fhe_kway_rotation_indices(N). */
int fhe_kway_sort(fhe_ctx *ctx, const fhe_ct *x, int k, int M, int dg, int df, fhe_ct **out);
/* the same with bootstrapping (KWaySort235Test's context, tests/k-way/
 * KWaySort235Test.cpp:18-51): checkLevelAndBoot and compositeSign's lazy
 * bootstrap (src/sign.cpp:164-170) call fhe_bootstrap(boot); boot's slots
 * must equal x's.  bootstraps (may be NULL): checkLevelAndBoot bootstraps done. */
int fhe_kway_sort_boot(fhe_ctx *ctx, const fhe_ct *x, int k, int M, int dg, int df, fhe_boot *boot,
                       int *bootstraps, fhe_ct **out);
/* SortUtils::fcnL (kk = 1: out[0] = fcnL(x0, x1, cmp0) = cmp*(x0-x1)+x1,
 * src/k-way/SortUtils.cpp:5-16) or the kk-sorter for kk = 2..5
 * (SortUtils.cpp:32-208): nx = kk inputs, ncmp = kk(kk-1)/2 comparison
 * ciphertexts in SortUtilsTest's order (a>b, a>c, ..., tests/k-way/
 * SortUtilsTest.cpp:68-260); out receives kk ciphertexts in ascending order. */
/* EvalUtils::checkLevelAndBoot(ctxt, level, multDepth) (src/k-way/EvalUtils.cpp:57-86), the
 * k-way sorter's own level check: *out = x bootstrapped with `boot` when fewer than need + 1
 * levels remain (FHE_EDEPTH without a bootstrapper), else a new handle sharing x's
 * storage (free both; fhe_ct_set_slots on one shows on the other); *booted = 1 / 0.
 * checkLevelAndBoot2 (:88-94) is this call on each of its two ciphertexts. */
int fhe_check_level_and_boot(fhe_ctx *ctx, const fhe_ct *x, int need, fhe_boot *boot, int *booted, fhe_ct **out);
/* k = 5 stages compare x against two rotations of itself.  on != 0: the pair
 * runs as one 2-member stack on the context's engine -- one compare, its lazy
 * bootstraps taken on the stack, and a pair that the level check has to
 * bootstrap refreshed in one pass -- instead of two one-ciphertext chains on two
 * lanes (fhe_set_sort_lanes is then not used by the k-way sorter).  The output
 * words do not depend on it.  Initial value: FHE_KWAY_STACK from the environment
 * at fhe_ctx_create, else 0. */
int fhe_set_kway_stack(fhe_ctx *ctx, int on);
int fhe_kway_sorter(fhe_ctx *ctx, int kk, const fhe_ct *const *x, int nx, const fhe_ct *const *cmp, int ncmp,
                    fhe_ct **out);
/* kwaySort::sortType(k, M, stage) -> (m, logDist, slope) (src/k-way/Masking.cpp:25-48) */
int fhe_kway_sort_type(int k, int M, int stage, int *m, int *log_dist, int *slope);
/* number of stages, M + M(M-1)/2 * ceil(k/2) (src/k-way/Sorter.cpp:290); < 0 on error */
int fhe_kway_stage_count(int k, int M);
/* kwaySort::getRotateDistance (src/k-way/Masking.cpp:155-165); < 0 on error */
int fhe_kway_rotate_distance(int k, int log_dist, int slope);
/* kwaySort::genIndices (src/k-way/Masking.cpp:50-146): group[i] = indices[0][i],
 * position[i] = indices[1][i] for i < num_slots */
int fhe_kway_gen_indices(int num_slots, int k, int M, int m, int log_dist, int slope, int32_t *group,
                         int32_t *position);
/* KWayAdapter<N>::getSizeParameters rotation set (+-2^i < N, src/kway_adapter.h:45-49);
 * returns the count (< 0: error) */
int fhe_kway_rotation_indices(int N, int32_t *rots, int max_rots);

/* ---------------------------------------------------- CKKS bootstrapping */
/* FHECKKSRNS::EvalBootstrapSetup(levelBudget, {0, 0}, numSlots) as the
 * reference calls it (tests/k-way/KWaySort235Test.cpp:46-47, level budgets from
 * KWayAdapter<N>::getSizeParameters, src/kway_adapter.h:55-62).  Sparse packing:
 * slots a power of two in [2, n/4].  EvalMod range K (|t/q0| <= K; 512 for the
 * uniform ternary secret), r double angles, cosine degree (EvalMod coefficients
 * evalmod_k<K>r<r>_<degree>.f64 in the coefficient directory), correction_bits:
 * the message is scaled to q0 2^-bits before ModRaise.  Zero fields take the
 * defaults {budget 4/4, K 512, r 6, degree 88, bits 10}.  The bootstrapper
 * refers to ctx: destroy it first. */
typedef struct {
    int slots;
    int level_budget_enc, level_budget_dec;
    int K, r, degree, correction_bits;
} fhe_boot_params;
int fhe_boot_create(fhe_ctx *ctx, const fhe_boot_params *p, fhe_boot **out);
int fhe_boot_destroy(fhe_boot *b);
/* EvalBootstrapKeyGen(sk, numSlots) (KWaySort235Test.cpp:48): the rotation keys
 * of the trace and linear transforms plus the conjugation key, on the GPU */
int fhe_boot_keygen(fhe_boot *b);
/* the rotation indices fhe_boot_keygen generates (returns the count, < 0: error) */
int fhe_boot_rotation_indices(const fhe_boot *b, int32_t *rots, int max_rots);
/* output level of fhe_bootstrap (levels the bootstrap consumes from the top) */
int fhe_boot_depth(const fhe_boot *b);
/* CryptoContext::EvalBootstrap(ct) (src/k-way/EvalUtils.cpp:76, src/sign.cpp:168):
 * x at level <= mult_depth - 1 with the setup's slots; out at fhe_boot_depth.
 * x may be a stack (fhe_ct_stack) of any size: its members are refreshed in the
 * same kernel launches, the transforms' keys and plaintexts read once per block
 * of members, and member m of out holds, word for word, what fhe_bootstrap of
 * member m alone gives.  The same holds for fhe_bootstrap_stage and
 * fhe_check_level_and_boot. */
int fhe_bootstrap(fhe_boot *b, const fhe_ct *x, fhe_ct **out);
/* the stages alone (parity tests): 1 CoeffsToSlots of a raised ciphertext
 * (+ conjugate-add), 2 EvalMod, 3 SlotsToCoeffs, 4 ModRaise */
int fhe_bootstrap_stage(fhe_boot *b, const fhe_ct *x, int stage, fhe_ct **out);
/* bootstraps since the last fhe_reset_counters, over the context's engines:
 * out[0] = bootstrap passes run, out[1] = ciphertexts refreshed (a stack of B
 * counts as one pass and B ciphertexts) */
int fhe_boot_counters(fhe_ctx *ctx, uint64_t out[2]);
/* EvalConjugate-style keyed automorphism X -> X^(2n-1) */
int fhe_conjugate(fhe_ctx *ctx, const fhe_ct *a, fhe_ct **out);
/* keys of arbitrary galois elements g (odd, < 2n); load one generated elsewhere */
int fhe_gen_galois_keys(fhe_ctx *ctx, const uint64_t *g, int n);
int fhe_ctx_load_galois_key(fhe_ctx *ctx, uint64_t g, const uint64_t *key);
/* MakeCKKSPackedPlaintext of complex slot values at an explicit scale */
int fhe_pt_encode_complex(fhe_ctx *ctx, const double *re, const double *im, int len, int slots, int level,
                          double scale, fhe_pt **out);

/* ------------------------------------------------------ multi-GPU (RCCL) */
int fhe_comm_get_unique_id(uint8_t id[128]);
/* FHE_EINVAL, before RCCL is touched, unless 0 <= rank < world and world * q_max < 2^64
 * (the all-reduce sums u64 residues; world <= 16 at a 60-bit q0) */
int fhe_comm_init(fhe_ctx *ctx, const uint8_t id[128], int rank, int world);
int fhe_comm_destroy(fhe_ctx *ctx);
/* sum the ciphertext over all ranks (RCCL all-reduce u64 + per-limb mod q) */
int fhe_ct_allreduce(fhe_ctx *ctx, fhe_ct *ct);

/* ---------------------------------------------- kernel-level (parity) */
int fhe_ntt(fhe_ctx *ctx, uint64_t *host, int prime_index, int limbs, int inverse);
int fhe_modup(fhe_ctx *ctx, const uint64_t *d, int ell, uint64_t *ext);
int fhe_moddown(fhe_ctx *ctx, const uint64_t *in, int ell, uint64_t *out);
int fhe_automorph(fhe_ctx *ctx, const uint64_t *in, int limbs, uint64_t galois, uint64_t *out);
/* kernel-level parity of the multi-output sums of products (the Paterson-Stockmeyer leaves):
 * outs[g] = sum_i (K[g m + i] 2^sh[g m + i] mod q_l) xs[i], g < G, unrescaled at `level`, with the
 * constants as the integer pairs the kernels take instead of doubles (|K| <= 2^62, else
 * FHE_EINVAL).  Kc / shc ([G], or both NULL): + (Kc[g] 2^shc[g]) q_last mod q_l on c0 below the
 * last limb, the constant a following rescale turns into + Kc 2^shc.  Inputs above `level` or of
 * mixed batch sizes are refused.  Same tables, kernel selection and passes as the sums inside
 * fhe_cheb_ps. */
int fhe_linear_sums_raw(fhe_ctx *ctx, const fhe_ct *const *xs, int m, const int64_t *K, const uint8_t *sh, int G,
                        const int64_t *Kc, const uint8_t *shc, int level, fhe_ct **outs);
/* kernel-level parity: a_digit of key `kid` over all nq+K primes, [nall][n] to host */
int fhe_public_poly(fhe_ctx *ctx, const uint8_t seed[32], uint64_t kid, int digit, uint64_t *out);
/* Device-memory variants (SURVEY §8(b) fhe_ntt_fwd/inv, fhe_automorph): the
 * limbs are device pointers, the work is enqueued on `stream` (a hipStream_t;
 * NULL = the context stream) and the call returns without synchronising.
 * fhe_ntt_dev transforms, in place, `nlimbs` limbs over the consecutive primes
 * first_prime.. of `segments` polynomials (polynomial s at dev_limbs + s *
 * seg_stride words; layout [limb][n], NTT order as fhe_ntt).  The ring's
 * twiddle tables are the context's; the caller keeps the buffers alive until
 * the stream has run the work. */
int fhe_ntt_dev(fhe_ctx *ctx, uint64_t *dev_limbs, int first_prime, int nlimbs, int segments, uint64_t seg_stride,
                int inverse, void *stream);
int fhe_automorph_dev(fhe_ctx *ctx, const uint64_t *dev_in, int limbs, uint64_t galois, uint64_t *dev_out,
                      void *stream);
/* Process-wide choice of the sums-of-products kernels (PS linear sums = 1,
 * ModUp conversion = 2, fused ModDown+rescale conversion = 4): a set bit runs
 * that conversion on the i8 matrix cores (v_mfma_i32_16x16x64_i8),
 * a clear bit on the 64-bit VALU kernels.  The output words are the same
 * either way.  mask < 0 only queries.  Returns the previous mask (initially
 * FHE_MFMA from the environment, else the build default). */
int fhe_set_mfma_sums(int mask);
/* op counters: hmult, keyswitch, rotations, rescale, ptmult, constmult, and
 * the op-level algorithmic HBM bytes of SURVEY §8(d) (HMult, rotation, ct x pt,
 * ct x const, add, linear sum formulas, each op at its own level) */
int fhe_counters(fhe_ctx *ctx, uint64_t out[7]);
int fhe_reset_counters(fhe_ctx *ctx);
/* DirectSort's public masks and checking vectors: cache != 0 (default) encodes
 * each once per context and keeps it; cache == 0 re-encodes all of a sort's
 * masks on the device at the start of every sort, as the reference encodes
 * them on every use (src/sort_algo.h:341-342, 714-716) */
int fhe_set_mask_cache(fhe_ctx *ctx, int cache);
/* sharded sorts' partial-sum exchanges since the last fhe_reset_counters:
 * out = {host nanoseconds inside them (header + data all-reduce, measured from a
 * drained stream to the reduced data), exchanges}.  The reference's reduction
 * points are the rank sums after its batch loops (src/sort_algo.h:489-490,
 * 740-741); a bench splits a rank's wall into compute and collective with it. */
int fhe_collective_stats(fhe_ctx *ctx, uint64_t out[2]);
int fhe_sync(fhe_ctx *ctx);
/* enqueue an empty marker kernel (k_region_begin if begin != 0, else
 * k_region_end) on the context stream: it delimits a measured region in a
 * rocprofv3 kernel trace or PMC pass (bench.py FHE_PROF_REGION=1) */
int fhe_region_marker(fhe_ctx *ctx, int begin);
/* opaque hipStream_t of the context (for event timing by the caller) */
void *fhe_stream(fhe_ctx *ctx);
/* time `iters` launches of one hot kernel ("ks_inner", "ntt_fwd",
 * "modup_convert") with HIP events on the context stream, shaped as a key
 * switch at `limbs` Q limbs: average ms and algorithmic bytes/launch */
int fhe_time_kernel(fhe_ctx *ctx, const char *name, int limbs, int iters, double *avg_ms, double *bytes);
/* device memory pool of the context: release cached blocks to HIP; bytes in
 * use, cached, and the peak in use since creation */
int fhe_pool_trim(fhe_ctx *ctx);
/* process-wide host costs since the last reset: out = {plaintext encodes, seconds
 * in them (host special FFT, rounding, upload, NTT), device allocations that
 * missed the pools' caches, seconds in hipMalloc} -- the cold-sort breakdown */
int fhe_host_stats(double out[4]);
int fhe_host_stats_reset(void);
int fhe_pool_stats(fhe_ctx *ctx, uint64_t *live, uint64_t *cached, uint64_t *peak);
/* live kernel clock over real work: after start, every NTT pass launched by
 * this process is bracketed by HIP events on its stream; stop writes JSON
 * {"<kernel>": {"launches": c, "ms": total, "bytes": algorithmic}, ...} into
 * json (cap bytes, NUL-terminated, truncated if short; *needed = full size) */
int fhe_kernel_clock_start(fhe_ctx *ctx);
int fhe_kernel_clock_stop(fhe_ctx *ctx, char *json, size_t cap, size_t *needed);

/* ------------------------------------------------------------ wire format
 * The reference's CLI (src/sort.h:31-74, 97-102; src/main.cpp:9-44) reads the
 * crypto context, public key, eval-mult key, eval-automorphism (rotation) keys
 * and input ciphertext from files and writes the sorted ciphertext back, via
 * OpenFHE's Serial API in SerType::BINARY.  These calls do the same in the
 * engine's own format (fhe-sorting_amd/csrc/wire/wire.hpp):
 * checksummed, tied to the context's modulus chain, validated before anything
 * is loaded.  Errors: FHE_EIO (open / read / write / corrupt / not a wire file),
 * FHE_EINVAL (wrong object kind, other context, out-of-range residues). */
typedef struct {
    uint32_t kind;     /* 1 context, 2 public key, 3 eval-mult key, 4 automorphism keys, 5 ciphertext, 6 secret key,
                          7 seeded eval-mult key, 8 seeded automorphism keys */
    uint32_t version;
    uint64_t params_id, log_n, nq, K, body_words;
} fhe_wire_info;
int fhe_wire_inspect(const char *path, fhe_wire_info *info);  /* host only: header + checksum */
/* Serial::SerializeToFile / DeserializeFromFile(ccLocation, m_cc) (src/sort.h:34) */
int fhe_serialize_context(fhe_ctx *ctx, const char *path);
int fhe_deserialize_context(const char *path, int device, fhe_ctx **out);
/* ... (pubKeyLocation, m_PublicKey) (src/sort.h:40) */
int fhe_serialize_public_key(fhe_ctx *ctx, const char *path);
int fhe_deserialize_public_key(fhe_ctx *ctx, const char *path);
/* the client side's secret key (the reference's tests keep it in memory) */
int fhe_serialize_secret_key(fhe_ctx *ctx, const char *path);
int fhe_deserialize_secret_key(fhe_ctx *ctx, const char *path);
/* SerializeEvalMultKey / DeserializeEvalMultKey (src/sort.h:46-55) */
int fhe_serialize_eval_mult_key(fhe_ctx *ctx, const char *path);
int fhe_deserialize_eval_mult_key(fhe_ctx *ctx, const char *path);
/* SerializeEvalAutomorphismKey / DeserializeEvalAutomorphismKey (src/sort.h:57-67):
 * every galois key of the context (rotations, conjugation); count: keys loaded */
int fhe_serialize_eval_automorphism_key(fhe_ctx *ctx, const char *path);
int fhe_deserialize_eval_automorphism_key(fhe_ctx *ctx, const char *path, int *count);
/* the same keys without their uniform halves (wire kinds 7 and 8: the b halves and the
 * public seed, half the bytes): FHE_EINVAL, naming the key, unless every key to be
 * written was generated under a public seed and all under the same one.  The two
 * deserialize calls above read either format, going by the file's header, and expand
 * the uniform halves on the GPU. */
int fhe_serialize_eval_mult_key_seeded(fhe_ctx *ctx, const char *path);
int fhe_serialize_eval_automorphism_key_seeded(fhe_ctx *ctx, const char *path);
/* Serial::{Deserialize,Serialize}ToFile of a ciphertext (src/sort.h:69-73, 97-102) */
int fhe_serialize_ciphertext(fhe_ctx *ctx, const fhe_ct *ct, const char *path);
int fhe_deserialize_ciphertext(fhe_ctx *ctx, const char *path, fhe_ct **out);

#ifdef __cplusplus
}
#endif
#endif /* FHE_GPU_H */
