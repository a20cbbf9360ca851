// C++ call surface of the rank-sort comparator hot path, MI355X edition.
//
// Mirrors the reference's interface (names, argument meaning, error
// behaviour) so a caller of oksuman/FHE-Sorting finds the same entry points:
//   enum SignFunc, CompositeSignConfig, SignConfig      src/sign.h:6-32
//   compositeSign<n>(), sign()                          src/sign.h:35-41
//   Comparison::compare / indicator                     src/comparison.h:81-101
//   DecomposeAlgo, Step, Decomposer<N>                  src/rotation.h:12-166
//   RotationComposer<N>::rotate                         src/rotation.h:193-233
//   DirectSort<N>::{getSizeParameters, constructRank,
//                   rotationIndexCheckN, sort}          src/sort_algo.h:61-774
// Every operation executes on the GPU through fhe::Engine (engine.hpp); the
// templates are thin wrappers over runtime-N implementations.
#pragma once
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <tuple>
#include <vector>

#include "../engine/engine.hpp"

namespace fhe {

enum class SignFunc { CompositeSign = 0, SignumPolycircuit = 1, Tanh = 2, NaiveDiscrete = 3 };

struct CompositeSignConfig {
    int n, dg, df;
    CompositeSignConfig(int n_, int dg_, int df_) : n(n_), dg(dg_), df(df_) {}
};
struct SignConfig {
    CompositeSignConfig compos{0, 0, 0};
    int multDepth = 100;  // src/sign.h:27-28
    // compositeSign's lazyBootstrap (src/sign.cpp:164-170): when set, g_n / f_n
    // run on a bootstrapped input whenever fewer than depth + 2 levels remain
    // (the context's depth is the reference's Cfg.multDepth)
    std::function<CtPtr(const Ciphertext &)> boot;
    // optional: several ciphertexts (any levels) bootstrapped in one pass, the
    // result a stack in the order given (Bootstrapper::evalBootstrapMany)
    std::function<CtPtr(const std::vector<const Ciphertext *> &)> bootMany;
    SignConfig() = default;
    explicit SignConfig(CompositeSignConfig c) : compos(c) {}
    SignConfig(CompositeSignConfig c, int depth) : compos(c), multDepth(depth) {}
};

// Chebyshev series sum c_0/2 + sum_{i>=1} c_i T_i((2x-a-b)/(b-a)) by
// Paterson-Stockmeyer; replaces OpenFHE EvalChebyshevSeriesPS.  The split is
// cc.ps_split: OpenFHE's (default) or the engine's power-of-two one.
CtPtr evalChebyshevSeriesPS(Engine &cc, const Ciphertext &x, const std::vector<double> &coeffs, double a,
                            double b);
// levels evalChebyshevSeriesPS consumes for a degree-d series (OpenFHE split /
// given split)
int chebPSDepth(int degree);
// true iff evalChebyshevSeriesPS under PS_SPLIT_OPENFHE evaluates these
// coefficients with OpenFHE's division tree (false: the power-of-two fallback
// of an ill-conditioned or degree < 5 series)
bool chebPSUsesOpenFHE(const std::vector<double> &coeffs);
int chebPSDepthSplit(int degree, int split);

CtPtr compositeSignN(Engine &cc, const Ciphertext &x, int n, const SignConfig &cfg);
template <int n>
CtPtr compositeSign(const Ciphertext &x, Engine &cc, const SignConfig &cfg) {
    return compositeSignN(cc, x, n, cfg);
}
CtPtr sign(const Ciphertext &x, Engine &cc, SignFunc func, const SignConfig &cfg);

class Comparison {
  public:
    CtPtr compare(Engine &cc, const Ciphertext &a, const Ciphertext &b, SignFunc f, const SignConfig &cfg);
    // c1 = compare(a, b1), c2 = compare(a, b2), word for word, with the two sign
    // chains run as one 2-member stack from the first point at which they sit at
    // one level (at once when b1 and b2 do; otherwise after the first lazy
    // bootstrap both need, taken in one pass through cfg.bootMany); c1, c2 are
    // then member views of that stack
    void compare2(Engine &cc, const Ciphertext &a, const Ciphertext &b1, const Ciphertext &b2, SignFunc f,
                  const SignConfig &cfg, CtPtr &c1, CtPtr &c2);
    CtPtr indicator(Engine &cc, const Ciphertext &x, double c, SignFunc f, const SignConfig &cfg);
};

enum class DecomposeAlgo { NAF = 0, BNAF = 1, BINARY = 2 };
struct Step {
    int value;
    int stepSize;
};

class DecomposerN {
  public:
    DecomposerN(int N, std::vector<int> rot);
    std::vector<Step> decompose(int rotation, int wrapN, DecomposeAlgo algo) const;
    const std::vector<int> &getRotIndices() const { return rotIndices; }
    int N, maxDecomposed;
    std::vector<int> rotIndices;
};
template <int SIZE>
class Decomposer : public DecomposerN {
  public:
    explicit Decomposer(std::vector<int> rot) : DecomposerN(SIZE, std::move(rot)) {}
};

class RotationComposerN {
  public:
    RotationComposerN(Engine &cc, int N, const std::vector<int> &rotIndices,
                      DecomposeAlgo algo = DecomposeAlgo::BINARY);
    CtPtr rotate(const Ciphertext &in, int rotation);
    // several rotations of one input; single keyed steps share one ModUp
    std::vector<CtPtr> rotateMany(const Ciphertext &in, const std::vector<int> &rotations);
    // member m of the batch `in` rotated by rotations[m] through the same keyed
    // steps rotate() takes; step j of every member that has one runs in one
    // multi-key launch sequence (Engine::rotate_members).  Same words as
    // rotate() member by member.
    std::vector<CtPtr> rotateMembers(const Ciphertext &in, const std::vector<int> &rotations);
    Engine &cc;
    DecomposerN dec;
    DecomposeAlgo algo;
    std::set<int> avail;
};
template <int SIZE>
class RotationComposer : public RotationComposerN {
  public:
    RotationComposer(Engine &cc, const std::vector<int> &rot, DecomposeAlgo a = DecomposeAlgo::BINARY)
        : RotationComposerN(cc, SIZE, rot, a) {}
};

// src/rotation.h:168-191
struct RotationStats {
    size_t fastRotationCount = 0, normalRotationCount = 0, totalRotationCount = 0, cacheHits = 0, cacheMisses = 0;
    void reset() { *this = RotationStats(); }
};

// RotationTree<N> (src/rotation.h:240-358): rotations by any k as paths of
// keyed steps in a prefix tree; every node's rotated ciphertext is cached, and
// the children of a node are rotations of one ciphertext, so they share one
// ModUp.  The reference computes a child on first use with
// EvalFastRotation(node precompute); here the first use of any child of a
// node computes all of that node's built children in one hoisted launch
// sequence (fhe_rotate_hoisted) -- hoisted and single rotations are
// bit-identical in this engine, so results do not depend on the order of
// requests.  As in the reference, the cache belongs to the first input
// rotated: one tree per input ciphertext.
class RotationTreeN {
  public:
    RotationTreeN(Engine &cc, int N, const std::vector<int> &rotIndices, DecomposeAlgo algo = DecomposeAlgo::NAF);
    void buildTree(int start, int end);
    CtPtr treeRotate(const Ciphertext &input, int rotation);
    const RotationStats &getStats() const { return stats; }

  private:
    struct Node {
        int stepSize;
        Node *parent;
        std::map<int, std::unique_ptr<Node>> children;
        std::vector<int> finalValues;
        CtPtr rotated;
        Node(int s, Node *p) : stepSize(s), parent(p) {}
    };
    void addToTree(Node *node, const std::vector<Step> &steps, size_t i, int value);
    CtPtr traverse(const CtPtr &input, Node *node, const std::vector<Step> &steps, size_t i);
    Engine &cc;
    DecomposerN dec;
    DecomposeAlgo algo;
    std::unique_ptr<Node> root;
    RotationStats stats;
};
template <int SIZE>
class RotationTree : public RotationTreeN {
  public:
    RotationTree(Engine &cc, const std::vector<int> &rot, DecomposeAlgo a = DecomposeAlgo::NAF)
        : RotationTreeN(cc, SIZE, rot, a) {}
};

struct SortShape {
    int N, num_partition, num_batch, num_slots, np;
};
void directSortSizeParameters(int N, int &multDepth, std::vector<int> &rotations);
// the hybrid sort test's parameters (tests/DirectSortHTest.cpp:23-104, ring 2^17)
void hybridSortSizeParameters(int N, int &multDepth, std::vector<int> &rotations);
SortShape rankShape(int N, int max_batch);
SortShape checkShape(int N, int max_batch);
// The all-pairs layout of a left table of Nl rows against a right table of Nr
// rows, both powers of two: with N = max(Nl, Nr),
// n = min(Nl, Nr) and P_ the square shape's partitions for N, P' = min(P_, n)
// partitions, n / P' batches, N P' slots, np = the square's baby steps for (N, P').
// Slot s of batch b pairs left row (s mod N) mod Nl with right row
// (s mod N + t) mod Nr, t = b P' + s / N < n.  Nl = Nr gives rankShape(N, max_batch).
SortShape pairShape(int Nl, int Nr, int max_batch);
// rounds of the residue fold that collects a left row's sum from the slots
// i = e mod Nl when Nl < Nr: log2(Nr / Nl), else 0
int pairFoldSteps(int Nl, int Nr);
// Layout of an order-statistic select of k targets over num_slots = N P_ slots
// (DirectSortN::selectColumns): cap = P_ - 1 targets per member (1 when P_ = 1);
// target p belongs to member p / cap and owns the cyclic window of N slots from
// start[p] = ((p % cap) (N + 1) + (p / cap) cap) mod num_slots on.  The windows of
// one member are disjoint, start[p] = p mod N, and every window holds each
// residue mod N once.  Returns the member count ceil(k / cap); member / start
// (optional) receive k entries.  Throws std::invalid_argument on a bad shape.
int selectLayout(int N, int num_slots, int k, std::vector<int> *member, std::vector<int> *start);
// Levels of DirectSortN::groupSums for keys at key_level under the composite sign
// (n, dg, df): sign_depth levels for the sign (3 per g_3 / f_3, 4 per f_4, g_4's
// series depth under `ps_split`; g runs once even when dg = 0), the differences
// at diff_level = key_level + 1 (one masked sum below the keys), the match
// indicator at match_level = diff_level + sign_depth, the columns brought to
// match_level - 1 before their own masked sum, so a column may sit at
// col_max_level = match_level - 2 at most, and every output at
// out_level = match_level + 1: where constructRank ends.  Throws
// std::invalid_argument on a negative level or a sign the GPU path lacks.
struct GroupSumLevels {
    int sign_depth, diff_level, match_level, col_max_level, out_level;
};
GroupSumLevels groupSumLevels(int key_level, int n, int dg, int df, int ps_split = PS_SPLIT_OPENFHE);

// Levels of DirectSortN::lexRank for nkeys keys (2..4) at key_level under the
// composite sign (n, dg, df): the differences at diff_level = key_level + 1, every
// sign output at sign_level = diff_level + sign_depth, one level per Horner step
// and one for the closing 2^-nkeys, so the rank ends at rank_level = sign_level +
// nkeys: nkeys - 1 levels below constructRank's.  Throws std::invalid_argument on
// a key count outside 2..4, a negative level or a sign the GPU path lacks.
struct LexRankLevels {
    int sign_depth, diff_level, sign_level, rank_level;
};
LexRankLevels lexRankLevels(int key_level, int nkeys, int n, int dg, int df, int ps_split = PS_SPLIT_OPENFHE);

// Levels of DirectSortN::windowSums for keys at key_level and nfactors pair
// indicators (2..4: the partition keys, plus one for an order key) under the
// composite sign (n, dg, df): the differences at diff_level = key_level + 1, every
// sign output at match_level = diff_level + sign_depth, the indicators' product
// after a tree of ceil(log2 nfactors) products at prod_level, the columns brought
// to prod_level - 1 before their own masked sum, so a column may sit at
// col_max_level = prod_level - 2 at most, and every output at out_level =
// prod_level + 1.  Throws std::invalid_argument on a factor count outside 2..4, a
// negative level or a sign the GPU path lacks.
struct WindowSumLevels {
    int sign_depth, diff_level, match_level, prod_level, col_max_level, out_level;
};
WindowSumLevels windowSumLevels(int key_level, int nfactors, int n, int dg, int df, int ps_split = PS_SPLIT_OPENFHE);

// Levels of DirectSortN::gatherColumns for positions at pos_level over N rows: the
// differences at diff_level = pos_level + 1 (one masked sum below the positions),
// the series output (and the present flags) at series_level = diff_level + 1 +
// the doubled-sinc series' depth under `ps_split` (DirectSortN::indexSeriesLevel of
// diff_level), the columns brought to series_level - 1 before their own masked
// sum, so a column may sit at col_max_level = series_level - 2 at most, and every
// gathered column at out_level = series_level + 1.  Throws std::invalid_argument on
// a negative level, std::runtime_error where N has no coefficient table.
struct GatherLevels {
    int diff_level, series_level, col_max_level, out_level;
};
GatherLevels gatherLevels(int pos_level, int N, int ps_split = PS_SPLIT_OPENFHE);

// Sums a ciphertext's u64 limbs over ranks in place (device pointer, count
// u64); the engine reduces mod q afterwards.  nullptr = single rank.
using CtAllReduce = std::function<void(u64 *dev_data, size_t count)>;

// Independent work items i handled by this rank iff i % world == rank; partial
// sums combined by `allreduce`.
struct Shard {
    int rank = 0, world = 1;
    CtAllReduce allreduce;
    bool mine(size_t i) const { return world <= 1 || (int)(i % (size_t)world) == rank; }
};
// Combines per-rank partial sums of one ciphertext: a 4-word header
// (presence, level + 1, (level + 1)^2, limbs) is summed first so ranks that
// hold no partial agree on the level and contribute a zero ciphertext, and
// ranks whose partials disagree on level or limbs all fail with the same error
// instead of entering mismatched collectives; then the limbs are summed as u64
// and reduced mod q.  No-op for one rank.  A partial may be a stack of `batch`
// members (the same on every rank): one header, then all members' words in one
// all-reduce.
void reducePartial(Engine &cc, const Shard &sh, CtPtr &acc, int slots, int batch = 1);

// The u64 sum of `world` residues, each < q_max, must not wrap: world * q_max
// < 2^64 (world <= 16 for the 60-bit first prime).  Throws otherwise.
void checkShardWorld(const host::Params &P, int world);
struct ShardHeader {
    int level;
    size_t limbs;
};
ShardHeader checkShardHeader(const u64 h[4]);

class DirectSortN {
  public:
    DirectSortN(Engine &cc, int N, const std::vector<int> &rotIndices);
    CtPtr constructRank(const Ciphertext &x, SignFunc f, const SignConfig &cfg);
    CtPtr rotationIndexCheckN(const Ciphertext &rank, const Ciphertext &x);
    CtPtr sort(const Ciphertext &x, SignFunc f, const SignConfig &cfg);
    // Records: out[p] = rotationIndexCheckN(rank, *cols[p]) word for word, with the
    // doubled-sinc series (which depends on the rank alone) evaluated once per
    // batch chunk and multiplied into every column in one stacked product
    // (Engine::mul_columns); the masked sums, giant steps, lane partials, the
    // shard reduction and the fold then run on column stacks.  A column deeper
    // than the series output (indexSeriesLevel) is refused before any work.
    // With tied keys the columns mix exactly as the key does (tests/tie_model.py)
    // unless the rank was built with `tiebreak` set.
    std::vector<CtPtr> rotationIndexCheckColumns(const Ciphertext &rank, const std::vector<const Ciphertext *> &cols);
    // constructRank(key), then rotationIndexCheckColumns
    std::vector<CtPtr> sortColumns(const Ciphertext &key, const std::vector<const Ciphertext *> &cols, SignFunc f,
                                   const SignConfig &cfg);
    // Order statistics: out[c] holds, at slot p < targets.size(), column c's value
    // at the element whose rank is targets[p] (any order, repeats allowed), and 0
    // in the other slots -- the project's own extension, not in the reference.
    // One group of N slots is dedicated to each target (selectLayout; DESIGN.md
    // "Order statistics"): the rank is subtracted from the target held constant on
    // that window, the index check's doubled-sinc series is evaluated once per
    // member (a ciphertext of num_slots = N P_ slots holds P_ - 1 targets), the
    // result is multiplied into every column (Engine::mul_columns), each window is
    // summed into its first slot by log2(N) rotations, the first slots of all
    // members are picked and added with one rescale
    // (Engine::mul_plain_sum_groups), and the sort's fold brings them to slot p.
    // Members run stacked in chunks of max_stack on the context's engine; the
    // words do not depend on the chunking.  Same depth and output level as the
    // sort; a column deeper than the series output is refused before any work.
    // Unsharded.  With tied keys the result mixes as the sort does
    // (tests/tie_model.py) unless the rank was built with `tiebreak` set.
    // cache_masks false: the call re-encodes its own plaintexts at its start.
    std::vector<CtPtr> selectColumns(const Ciphertext &rank, const std::vector<const Ciphertext *> &cols,
                                     const std::vector<int> &targets);
    // constructRank(key), then selectColumns
    std::vector<CtPtr> selectColumns(const Ciphertext &key, const std::vector<const Ciphertext *> &cols,
                                     const std::vector<int> &targets, SignFunc f, const SignConfig &cfg);
    // Group sums and lookups (the project's own extension): with
    // P = cols.size(), out[p] holds at slot e  sum_j [|kl_e - kr_j| < eps] cols[p]_j,
    // j over the N rows of the right table; want_count appends the count of
    // matching rows as out[P].  kr = kl is SUM / COUNT OVER (PARTITION BY key), the
    // row itself included; another table's key and columns give the LEFT JOIN
    // lookup, zero where no right key matches.  constructRank's all-pairs layout
    // with the shifted right key and the same shifted copies of the columns
    // (vecRotsOpt); the match indicator sign(d + eps) + sign(-d + eps) (2 or 0) of a
    // chunk of B batches is one sign over a 2 B stack (Engine::sub_pm_const_stacked)
    // and meets the columns, halved on their way to its level, in one stacked
    // product (Engine::mul_pairs); sums over batches are exact mod q, then the
    // rank's fold.  Needs equal keys equal up to noise far below eps, distinct keys
    // >= 2 eps apart, |kl_e - kr_j| + eps <= 1 and a sign configuration that
    // resolves eps (the tie-break's conditions).  Levels: groupSumLevels; a column
    // above col_max_level or a context without out_level levels is refused before
    // any work.  The words do not depend on max_stack, lanes, max_col_members or
    // cache_masks (false: the call re-encodes the cached masks at its start).
    // Unsharded; `tiebreak` has no effect.
    std::vector<CtPtr> groupSums(const Ciphertext &kl, const Ciphertext &kr, const std::vector<const Ciphertext *> &cols,
                                 double eps, bool want_count, SignFunc f, const SignConfig &cfg);
    // Lexicographic rank (the project's own extension): the rank of
    // row e among the N rows ordered by keys[0], then keys[1], ... (2..4 keys, most
    // significant first, single ciphertexts of N slots at one level).  With
    // d_l = K_l[e] - K_l[j] per pair: u_l = sign(d_l + eps), w_l = sign(d_l - eps) on the
    // leading keys, s = sign(d_{L-1} + E) on the last (E the tie-break offset when
    // `tiebreak` is set), T_{L-1} = s + 1, T_l = (u_l - w_l) T_{l+1} + 2^{L-1-l} (w_l + 1),
    // rank_e = 2^-L sum_j T_0 - c, c = 1 with the tie-break (the stable lexicographic
    // argsort rank) and 1/2 without (rows tied on every key behave as the plain
    // rank's ties).  constructRank's all-pairs layout with one set of baby steps
    // per key and the rank's own masks; a chunk of B = max(1, max_stack / (2 L - 1))
    // batches runs one sign over a (2 L - 1) B stack (Engine::sub_lex_stacked) and
    // the Horner steps as stacked products (Engine::mul_lex).  Needs values equal on
    // a leading key equal far below eps, distinct ones >= 2 eps apart, |d| + eps <= 1,
    // a sign configuration that resolves eps, and the tie-break's conditions on the
    // last key.  Levels: lexRankLevels; a context without rank_level levels is
    // refused before any work.  The words do not depend on max_stack, lanes or
    // cache_masks (false: the call re-encodes what it caches at its start).
    // Unsharded.  The result feeds rotationIndexCheckN / rotationIndexCheckColumns /
    // selectColumns as any rank does.
    CtPtr lexRank(const std::vector<const Ciphertext *> &keys, double eps, SignFunc f, const SignConfig &cfg);
    // Running sums (the project's own extension): with P = cols.size(),
    // out[p] holds at slot e  sum_j c_ej cols[p]_j, j over the N rows of the right
    // table; want_count appends sum_j c_ej as out[P].  The weight c_ej by mode:
    //   RunRows     (sign(kl_e - kr_j + E_ej) + 1) / 2, E the tie-break offset of §6.3 built
    //               from this call's eps (+eps where j <= e): the stable row order, ROWS
    //               UNBOUNDED PRECEDING with the row itself;
    //   RunLE       (sign(kl_e - kr_j + eps) + 1) / 2: kr_j <= kl_e, peers included (SQL's
    //               default RANGE frame, searchsorted side = right);
    //   RunLT       (sign(kl_e - kr_j - eps) + 1) / 2: kr_j < kl_e (searchsorted side = left);
    //   RunBetween  (sign(kl_e - kr_j + eps) - sign(lo_e - kr_j - eps)) / 2 with kl the upper
    //               bound: lo_e <= kr_j <= hi_e, both ends closed (the band join, the RANGE
    //               BETWEEN window).  lo is required in this mode and refused in the others.
    // groupSums' layout, levels (groupSumLevels), column preparation (halved on the
    // way to L_m - 1, sharing its cached masks), chunking, lanes and column groups.
    // A chunk of B batches is one sign over a B stack (2 B for RunBetween:
    // Engine::sub_bounds_stacked, or sub_add_plain_stacked for RunRows); the
    // indicator s + 1 (u - w) is formed as the stacked product loads it
    // (Engine::mul_pairs_const / mul_pairs_sub) and written out only for the count,
    // which is halved per batch as constructRank's compare is: in RunRows with
    // kr = kl, add_const(count, -1) is the tie-broken rank word for word.  Needs
    // equal keys equal far below eps, distinct keys (bounds included) >= 2 eps
    // apart, every sign argument within [-1, 1], a sign configuration that
    // resolves eps, and lo <= hi.  A column above col_max_level or a context
    // without out_level levels is refused before any work.  The words do not
    // depend on max_stack, lanes, max_col_members or cache_masks.  Unsharded;
    // `tiebreak` has no effect.
    enum RunMode { RunRows = 0, RunLE = 1, RunLT = 2, RunBetween = 3 };
    std::vector<CtPtr> runningSums(const Ciphertext &kl, const Ciphertext *lo, const Ciphertext &kr,
                                   const std::vector<const Ciphertext *> &cols, int mode, double eps, bool want_count,
                                   SignFunc f, const SignConfig &cfg);
    // Window sums (the project's own extension): the running sums
    // restricted to the rows that agree on every partition key.  With G = pl.size()
    // partition keys (1..3; pl[g] the left table's, pr[g] the right table's), an
    // optional order key (ol, orr, and olo for WinBetween) and P = cols.size(),
    // out[p] holds at slot e  sum_j c_ej cols[p]_j  and want_count appends sum_j c_ej,
    //   c_ej = prod_g [pl[g]_e = pr[g]_j] * [the mode selects j for e],
    // the partition indicator being (sign(d + eps) - sign(d - eps)) / 2 and the order
    // key's runningSums' for the mode (WinRows .. WinBetween = RunRows .. RunBetween);
    // WinGroup has no order key (GROUP BY a, b; the join on several keys) and needs
    // G >= 2.  F = G + (mode != WinGroup) factors, 2 <= F <= 4.  Levels:
    // windowSumLevels.  runningSums' layout, chunking (a chunk's sign runs over
    // 2 G + V members per batch, V = 0, 1 or 2), lanes and column groups; the
    // columns ride 2^-F on their way to prod_level - 1.  One
    // Engine::sub_window_stacked and one sign per chunk, the factor products on views
    // of the sign's stack (Engine::mul_sub_sub, mul_lex; an outer product of operands
    // at two levels takes sub and mul), then the column product.  Needs runningSums'
    // conditions on every key.  A column above col_max_level or a context without
    // out_level levels is refused before any work.  The words do not depend on
    // max_stack, lanes, max_col_members or cache_masks.  Unsharded; `tiebreak` has no
    // effect.
    enum WinMode { WinRows = 0, WinLE = 1, WinLT = 2, WinBetween = 3, WinGroup = 4 };
    std::vector<CtPtr> windowSums(const std::vector<const Ciphertext *> &pl, const std::vector<const Ciphertext *> &pr,
                                  const Ciphertext *ol, const Ciphertext *olo, const Ciphertext *orr,
                                  const std::vector<const Ciphertext *> &cols, int mode, double eps, bool want_count,
                                  SignFunc f, const SignConfig &cfg);
    // Gather by encrypted position (the project's own extension):
    // with P = cols.size() and K = offsets.size(), the output for column p and
    // offset o holds at slot e  sum_j delta(pl_e + o - pr_j) cols[p]_j, j over the N
    // right rows: the value of the right row standing o places after left row e's
    // position, zero where there is none.  pl = pr = a rank gives LAG / LEAD; an
    // encrypted iota as pr and encrypted indices as pl give the lookup col[idx].
    // pl and pr hold integers in [0, N) up to the noise a rank carries, the pr
    // distinct; |o| <= N - 1.  constructRank's all-pairs layout with the shifted
    // right positions and the same shifted copies of the columns; the oriented
    // differences of a chunk of B batches and the K offsets are one K B stack
    // (Engine::sub_offsets_stacked: pl - pr + o, negated for o < 0 so that it stays
    // above -N, where the doubled series fires too), the sort's 1/2N scaling and
    // doubled-sinc series run once over it, and it meets the columns in one
    // stacked product (Engine::mul_gather); sums over batches are exact mod q,
    // then the rank's fold.  want_present appends the same sums without the
    // column (1 where the neighbour exists), at the series' level.  sum_offsets
    // adds the K indicators of a batch before the product: one output per column,
    // the sum over the offsets (ROWS BETWEEN), and present the frame's row count.
    // Outputs: column-major (p K + k), then the present flags.  Levels:
    // gatherLevels; a column above col_max_level or a context without the levels
    // is refused before any work.  The words do not depend on max_stack, lanes,
    // max_col_members or cache_masks.  Unsharded; `tiebreak` has no effect.
    std::vector<CtPtr> gatherColumns(const Ciphertext &pl, const Ciphertext &pr,
                                     const std::vector<const Ciphertext *> &cols, const std::vector<int> &offsets,
                                     bool want_present, bool sum_offsets);
    // level of the index check's series output for a rank at rank_level: where
    // the product meets the column
    int indexSeriesLevel(int rank_level) const;
    // most members (columns x stacked batches) of one stacked column product;
    // more columns run in groups.  Results do not depend on it.
    int max_col_members = 64;
    // sort_hybrid (src/sort_algo.h:1050-1064): constructRank, then the MEHP24-style
    // matrix index check rotationIndexCheckHybrid (:893-1047); its num_batch^2
    // masks run stacked, blocks b shard over ranks like the rank-sort batches
    CtPtr rotationIndexCheckHybrid(const Ciphertext &rank, const Ciphertext &x);
    CtPtr sort_hybrid(const Ciphertext &x, SignFunc f, const SignConfig &cfg);
    int hybrid_max_array = 256;  // maxArraySize (:899)
    int hybrid_mask = 0;         // 0: by N as the reference; 1: scaled-sinc PS; 2: indicator (3,4,2); 3: (3,5,2)
    const std::vector<double> &sincCoefficients() const;

    int shard_rank = 0, shard_world = 1;
    CtAllReduce allreduce;
    Engine &cc;
    int N;
    RotationComposerN rot;
    int max_batch;
    // how many of this rank's batches run stacked through one compare / one PS
    // (every launch then carries that many ciphertexts; memory grows with it)
    int max_stack = 32;
    // concurrent lanes: the rank's batches are split over `lanes` host threads,
    // each driving a forked engine (own HIP stream and pool, shared keys)
    int lanes = 2;
    // public masks and checking vectors: true = encoded once per context and
    // kept; false = every sort re-encodes all of them on the device before it
    // starts (the reference encodes them on every use, src/sort_algo.h:341-342,
    // 714-716); masks are encoded on the device either way (FHE_HOST_MASKS=1:
    // the host encoder, A/B)
    bool cache_masks = true;
    // Tie-breaking for keys with equal values (0 = off, the
    // reference's rank).  eps in (0, 0.5): constructRank adds a public offset of
    // +-eps to every difference before the sign (Engine::sub_add_plain_stacked),
    // so the rank is the stable argsort rank #{x_j < x_e} + #{j < e : x_j = x_e}.
    // Needs distinct values >= 2 eps apart, a sign configuration that resolves
    // eps, and |x_i - x_j| + eps <= 1.  No extra depth; the output level is
    // unchanged.
    double tiebreak = 0.0;
    // Tables of different sizes (0, 0 = off, both tables hold N
    // rows): groupSums, runningSums, windowSums and gatherColumns pair a left table
    // of pair_left rows with a right table of pair_right rows, both powers of two
    // with max(pair_left, pair_right) = N.  Left operands come with pair_left
    // slots, right operands and columns with pair_right, outputs have pair_left.
    // The smaller table is viewed at the layout's slot count as it is (a tiling),
    // the walk runs min / P' batches (pairShape), and for pair_left < pair_right a
    // residue fold of pairFoldSteps rotations follows the partition fold.  No level
    // is consumed.  RunRows / WinRows are refused between unequal sizes.  The rank,
    // the lexicographic rank, the sort and the select do not read it.
    int pair_left = 0, pair_right = 0;

  private:
    struct Lane {
        Engine *eng;
        RotationComposerN *rot;
    };
    Lane lane(int l);
    // one result of work(lane, its batches) per lane, in lane order
    template <class F>
    auto run_lanes(const std::vector<int> &batches, F &&work);
    // One chunk of comparator batches inside a lane, as allPairs hands it to an
    // operator's indicator: the left operands' copies at num_slots, the right
    // operands shifted by every batch of the chunk (operand-major, B each; the
    // callback clears them once its differences are enqueued) and, where the
    // operator asked for them, the chunk's tie-break offsets.
    struct PairChunk {
        int B;
        const std::vector<const Ciphertext *> &dups;
        std::vector<CtPtr> &shifted;
        std::vector<const Plaintext *> offsets;
    };
    // What an operator hands allPairs: its operands, its sizes
    // and the three places where its predicate and its product differ.
    struct PairOp {
        const char *baby_phase, *batch_phase, *fold_phase;
        std::vector<const Ciphertext *> left, right;
        std::vector<const Ciphertext *> cols;  // empty: the column-free form (a rank)
        double col_scale = 1.0;                // every column enters as mul_const_to(col, col_scale, col_level)
        int col_level = 0;
        int sign_members = 1;  // members of a chunk's sign / series stack per batch: bounds the chunk
        int ind_members = 1;   // indicator members per batch that meet the columns: bounds the column groups
        bool want_count = false;
        bool sharded = false;   // constructRank alone: this rank's batches, then reducePartial
        double offs_eps = 0.0;  // > 0: the tie-break offsets E_b of this eps at offs_level
        int offs_level = 0;
        int n_left = 0, n_right = 0;  // rows of the two tables (0: N); unequal only without offsets, unsharded
        // the chunk's indicator stack (level asserted by the operator)
        std::function<CtPtr(Engine &, PairChunk &)> indicator;
        // adds the chunk's contribution to the lane's count / present partial
        // (the column-free form may consume the indicator in place)
        std::function<void(Engine &, CtPtr &ind, int B, CtPtr &cnt)> count;
        // indicator x the chunk's shifted columns (column-major, Pg columns of B)
        std::function<CtPtr(Engine &, const Ciphertext &ind, int B, const Ciphertext &cols, int Pg)> product;
        // on the folded count, inside the fold phase (a closing constant)
        std::function<void(CtPtr &cnt)> closing;
    };
    // The all-pairs layout every operator of DESIGN.md §6 walks: baby steps,
    // chunks of batches on the lanes, the lanes' partials added on the main
    // stream, the fold over the partitions (then, for n_left < n_right, over the
    // residues mod n_left).  Returns cols.size() * ind_members sums, then
    // (want_count) ind_members counts, each of n_left slots.
    std::vector<CtPtr> allPairs(const PairOp &op);
    // add(v, rotate(v, num_slots / 2^i)) over the partitions: the rank's fold
    void foldPartitions(CtPtr &v, const SortShape &s);
    // add(v, rotate(v, Nl 2^k)), k < pairFoldSteps: slot e gathers the slots e mod Nl
    void foldResidues(CtPtr &v, int Nl, int Nr);
    // the members of a folded stack as single ciphertexts of `slots` slots (0: N)
    std::vector<CtPtr> splitMembers(const CtPtr &v, int members, int slots = 0);
    // The two tables' row counts of a pair operator: (N, N) with the setting off,
    // else pair_left / pair_right, which must be powers of two >= 2 with the larger
    // one N; `rows_mode`: the operator's ROWS mode, refused between unequal sizes.
    struct PairTables {
        int nl, nr;
        bool set;
    };
    PairTables pairTables(const std::string &op, bool rows_mode) const;
    // with the setting on: `arg` must hold its table's row count of slots
    static void checkTableSlots(const std::string &op, const std::string &arg, const Ciphertext &c, bool left,
                                const PairTables &t);
    // columns per stacked product: the member bound over the largest chunk a lane stacks
    int perProduct(size_t batches, size_t chunk, int ind_members) const;
    // the lane partial of column groups, in column order
    static CtPtr stackGroups(Engine &E, const std::vector<CtPtr> &accs);
    // null, stack, slot count (slots >= 0: against `noun`, "the keys") and depth of every column
    static void checkColumns(const std::string &op, const std::string &noun,
                             const std::vector<const Ciphertext *> &cols, int slots, int max_level);
    CtPtr vecRotsOpt(Lane L, const std::vector<CtPtr> &baby, int num_partition, int num_slots, int np, int is);
    // vecRotsOpt of several batches: the giant-step rotations of all of them
    // (one amount per batch) run in shared launches (RotationComposerN::rotateMembers)
    std::vector<CtPtr> vecRotsOptMany(Lane L, const std::vector<CtPtr> &baby, int num_partition, int num_slots,
                                      int np, const std::vector<int> &iss);
    CtPtr blindRotationOptN(const std::vector<CtPtr> &masked, int num_slots, int np, int ib, int num_partition);
    // blindRotationOptN over a stacked `masked` (member m belongs to batch ibs[m]), summed over members
    CtPtr blindRotationStacked(Lane L, const std::vector<CtPtr> &masked, int num_slots, int np,
                               const std::vector<int> &ibs, int num_partition);
    // blindRotationStacked over P column groups: `masked` holds P * ibs.size()
    // members, column-major; the rotated members are summed per column into the
    // P-member stack acc (one grouped-sum launch per giant step)
    void blindRotationColumns(Lane L, const std::vector<CtPtr> &masked, int num_slots, int np,
                              const std::vector<int> &ibs, int P, int num_partition, CtPtr &acc);
    void reducePartial(CtPtr &acc, int slots, int batch = 1);
    std::vector<CtPtr> babySteps(const Ciphertext &x, int np);
    // encoded on the calling lane's engine, published once complete (thread-safe)
    const Plaintext &mask(Engine &E, int kind, int num_slots, int k, int rot, int level);
    // re-encode every cached mask in device batches on the main engine
    void refresh_masks();
    std::map<std::tuple<int, int, int, int, int>, PtPtr> mask_cache;
    std::mutex mask_mu;
    // the select's {C, K} plaintexts per (targets of the member, member, level of C, level of K)
    std::map<std::tuple<std::vector<int>, int, int, int>, std::array<PtPtr, 2>> select_cache;
    // the tie-break offsets E_b per (num_slots, batch, level, eps)
    std::map<std::tuple<int, int, int, double>, PtPtr> tiebreak_cache;
    // of the given batches for the offset eps (the rank passes `tiebreak`, the running sums their own)
    std::map<int, PtPtr> tiebreakOffsets(int num_slots, const std::vector<int> &batches, int level, double eps);
    std::vector<int> rot_indices;
    std::vector<std::unique_ptr<Engine>> lane_eng;
    std::vector<std::unique_ptr<RotationComposerN>> lane_rot;
};
template <int SIZE>
class DirectSort : public DirectSortN {
  public:
    DirectSort(Engine &cc, const std::vector<int> &rot) : DirectSortN(cc, SIZE, rot) {}
    static void getSizeParameters(int &multDepth, std::vector<int> &rotations) {
        directSortSizeParameters(SIZE, multDepth, rotations);
    }
};

// MEHP24 (Mazzone et al.) ranking / sorting, src/mehp24/mehp24_sort.h and
// mehp24_utils.h.  max_stack bounds how many independent compares /
// indicators run stacked in one batch (memory grows with it).
namespace mehp24 {
namespace utils {
// `sub` = sortLargeArrayFG's part length (256 in the reference)
std::vector<int> getRotationIndices(size_t N, size_t sub = 256);
// 0/1 row / column masks, encoded once per (kind, m, index, level, slots)
struct Masks {
    const Plaintext &get(Engine &cc, int kind, size_t m, size_t idx, int level, int slots);
    std::map<std::tuple<int, size_t, size_t, int, int>, PtPtr> cache;
};
CtPtr maskRow(Engine &cc, Masks &mk, const Ciphertext &c, size_t m, size_t row);
CtPtr maskColumn(Engine &cc, Masks &mk, const Ciphertext &c, size_t m, size_t col);
CtPtr replicateRow(Engine &cc, CtPtr c, size_t m);
CtPtr replicateColumn(Engine &cc, CtPtr c, size_t m);
CtPtr sumRows(Engine &cc, Masks &mk, CtPtr c, size_t m, bool mask, size_t row);
CtPtr sumColumns(Engine &cc, Masks &mk, CtPtr c, size_t m, bool mask);
CtPtr transposeRow(Engine &cc, Masks &mk, CtPtr c, size_t m, bool mask);
CtPtr transposeColumn(Engine &cc, Masks &mk, CtPtr c, size_t m, bool mask);
CtPtr signAdv(Engine &cc, CtPtr c, size_t dg, size_t df);
}  // namespace utils
CtPtr indicatorAdv(Engine &cc, const Ciphertext &c, double b, size_t dg, size_t df);
CtPtr sortFG(const Ciphertext &c, size_t vectorLength, SignFunc f, const SignConfig &cfg, uint32_t dg_i,
             uint32_t df_i, Engine &cc, int max_stack = 32);
// Multi-ciphertext sortFG shards its P(P+1)/2 pair compares and its P^2
// indicators over `sh` (one all-reduce per partial Cv / Ch / result sum);
// everything else is replicated.  The output does not depend on the sharding.
std::vector<CtPtr> sortFG(const std::vector<CtPtr> &c, size_t subVectorLength, SignFunc f, const SignConfig &cfg,
                          uint32_t dg_i, uint32_t df_i, Engine &cc, int max_stack = 32, const Shard &sh = Shard());
CtPtr sortLargeArrayFG(const Ciphertext &c, size_t totalLength, size_t subLength, SignFunc f,
                       const SignConfig &cfg, uint32_t dg_i, uint32_t df_i, Engine &cc, int max_stack = 32,
                       const Shard &sh = Shard());
struct Parameters {
    int multDepth = 0, logRingDim = 17, scaleModSize = 40, dnum = 3;
    int levels = 0;  // context depth: multDepth + 1 (input encrypted with encrypt_ext)
    SignConfig cfg;
    uint32_t dg_i = 0, df_i = 2;
    size_t subLength = 0;  // 0: sortFG on one ciphertext, else sortLargeArrayFG
    std::vector<int> rotations;
};
Parameters parameters(size_t N);
}  // namespace mehp24

// coefficient tables (generated offline by data/gen_doubled_sinc.py)
void setCoefficientDir(const std::string &dir);
const std::vector<double> &doubledSincCoefficients(int N);
const std::vector<double> &scaledSincCoefficients(int N);  // selectCoefficients<N>()
// bootstrapping's EvalMod cosine (data/gen_evalmod.py): evalmod_k<K>r<r>_<degree>.f64
const std::vector<double> &evalModCoefficients(int K, int r, int degree);

}  // namespace fhe
