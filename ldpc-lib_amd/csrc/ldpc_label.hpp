// ldpc_label.hpp -- upstream's generate_code (code_generation.cpp:35-115) on the device: label the edges of a protograph with circulant
// shifts so that the lifted graph reaches a target girth.  Included by ldpc_hip.hip; the host half also compiles with a plain C++
// compiler (tests/cpp/label_sanitize.cpp), the kernels only under hipcc.
//
//   host    equations(): the closed non-backtracking walks of length < target_girth, as upstream's spider finds them (graph_spider.h,
//           equations.cpp): for every root vertex all non-backtracking paths over vertices >= root, layer by layer; two paths of one
//           layer that end on the same vertex through different edges close a walk whose signed edge multiset (the BAG: + for column ->
//           row, - for row -> column, cancelling prefixes drop out) is either empty -- then no labelling can avoid that cycle and the
//           girth the tree allows drops to the walk's length -- or an equation.  Equations are a SET of bags after sign normalisation.
//           The table keeps, per equation, its terms over the RANDOM edges (a fixed edge's shift is 0 and contributes nothing).
//   device  a round of n attempts reads n * Er draws (Er random edges) from the mt19937 word tape (ldpc_mt.hpp).  A draw is libstdc++'s
//           uniform_int_distribution<int>(0, M - 1): the tempered word w is REJECTED iff (uint32)(w * M) < 2^32 mod M, else the value is
//           (w * M) >> 32 (bits/uniform_int_dist.h, _S_nd).  mark_kernel lists the rejected words of the round (rare: < M / 2^32 per
//           word), sort_kernel orders the list, and draw j of the round is word j + #{k : R[k] - k <= j}.
//           check_kernel: one attempt per lane, the wave's shifts in LDS as [edge][lane] int16 (rows padded by one dword so that the
//           wave's coalesced fill does not hit one bank), the equation table walked in the same order by all lanes (wave-uniform,
//           scalar loads), the walk ends when no lane of the wave is alive.  Divisibility by M is an exact reciprocal multiply.
//           Survivors leave as one 64-bit ballot mask per wave.  select_kernel walks the masks in order, applies upstream's
//           equal-columns test (over the column pairs with equal supports) to the survivors only, writes the first labellings that pass and notes where the generator stands.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

namespace ldpc_label {

// Limits (LDPC_HIP_EUNSUPPORTED beyond them).  The equation count grows roughly with (degree - 1)^(g / 2) per root: 5200 for the
// 16 x 32 Appendix C protograph at g = 8, millions at g = 12.  2^20 equations (at most g - 2 terms of 4 bytes each) keep the table
// below 256 MiB and its enumeration within seconds; a layer of the path tree is cut off at 2^22 nodes for the same reason.
constexpr int kMaxGirth = 64;                 // multiplicities fit 8 bits, |sum| < 62 * 32767 fits the reciprocal below
constexpr long long kMaxEquations = 1 << 20;
constexpr long long kMaxLayerNodes = 1 << 22;
constexpr int kMaxRandomEdges = 480;          // [edge][lane] int16 rows of 132 bytes: 63 360 bytes of LDS per wave
constexpr int kRowStride = 66;                // int16 per LDS row: 64 lanes + one dword of padding

typedef std::vector<std::pair<int, int>> Bag;   // (edge, multiplicity != 0), edges ascending

struct Table {
    int tree_girth = 0;
    int n_equations = 0;
    int n_edges = 0, n_random = 0;
    bool never_accepts = false;          // an equation without a random term: its sum is 0 whatever is drawn
    std::vector<int32_t> eq_begin;       // [n_equations + 1] into the term arrays
    std::vector<int32_t> term_edge;      // index among the random edges (edge order: column by column, rows ascending)
    std::vector<int32_t> term_mult;      // signed multiplicity, never 0
    std::vector<int32_t> cell;           // [nh][rh] column by column: -1 empty, -2 fixed (shift 0), else index among the random edges
    long long refused_count = 0;         // > 0: the enumeration stopped at this many equations / nodes
    const char *refused_what = "";
};

inline void bag_add(Bag &b, int edge, int sign) {
    Bag::iterator it = std::lower_bound(b.begin(), b.end(), std::make_pair(edge, -0x7fffffff));
    if (it != b.end() && it->first == edge) {
        it->second += sign;
        if (it->second == 0) b.erase(it);
    } else {
        b.insert(it, std::make_pair(edge, sign));
    }
}

// a - b
inline void bag_diff(const Bag &a, const Bag &b, Bag &out) {
    out.clear();
    size_t i = 0, j = 0;
    while (i < a.size() || j < b.size()) {
        if (j == b.size() || (i < a.size() && a[i].first < b[j].first)) out.push_back(a[i++]);
        else if (i == a.size() || b[j].first < a[i].first) { out.push_back(std::make_pair(b[j].first, -b[j].second)); ++j; }
        else {
            const int m = a[i].second - b[j].second;
            if (m) out.push_back(std::make_pair(a[i].first, m));
            ++i; ++j;
        }
    }
}

// proto [rh][nh] row-major: 0 empty, 1 random shift, any other positive value shift 0.  Returns false when a limit was hit
// (t.refused_count, t.refused_what).
inline bool equations(int rh, int nh, const int16_t *proto, int target_girth, Table &t) {
    struct Arc { int edge, to, sign; };
    struct Node { int vertex, edge; Bag bag; };
    const int V = nh + rh;
    std::vector<std::vector<Arc>> adj((size_t)V);
    std::vector<int> random_index;
    t = Table();
    t.cell.assign((size_t)nh * rh, -1);
    for (int j = 0; j < nh; ++j)
        for (int i = 0; i < rh; ++i) {
            const int v = proto[(size_t)i * nh + j];
            if (v <= 0) continue;
            const int e = t.n_edges++;
            adj[(size_t)j].push_back(Arc{e, nh + i, +1});
            adj[(size_t)(nh + i)].push_back(Arc{e, j, -1});
            random_index.push_back(v == 1 ? t.n_random++ : -1);
            t.cell[(size_t)j * rh + i] = v == 1 ? t.n_random - 1 : -2;
        }
    int tg = target_girth;
    std::map<Bag, int> found;   // normalised bag -> length of the shortest walk that has it
    std::vector<Node> layer, next;
    std::vector<std::vector<int>> by_vertex((size_t)V);
    Bag sum;
    for (int root = 0; root < V; ++root) {
        layer.assign(1, Node{root, -1, Bag()});
        for (int d = 1; 2 * d < tg && !layer.empty(); ++d) {
            next.clear();
            for (const Node &n : layer)
                for (const Arc &a : adj[(size_t)n.vertex]) {
                    if (a.edge == n.edge || a.to < root) continue;
                    if ((long long)next.size() >= kMaxLayerNodes) {
                        t.refused_count = (long long)next.size(); t.refused_what = "paths in one layer of the tree";
                        return false;
                    }
                    next.push_back(Node{a.to, a.edge, n.bag});
                    bag_add(next.back().bag, a.edge, a.sign);
                }
            for (std::vector<int> &b : by_vertex) b.clear();
            for (size_t k = 0; k < next.size(); ++k) by_vertex[(size_t)next[k].vertex].push_back((int)k);
            for (const std::vector<int> &b : by_vertex)
                for (size_t q = 1; q < b.size() && 2 * d < tg; ++q)
                    for (size_t p = 0; p < q && 2 * d < tg; ++p) {
                        const Node &lo = next[(size_t)b[p]], &hi = next[(size_t)b[q]];
                        if (lo.edge == hi.edge) continue;
                        bag_diff(hi.bag, lo.bag, sum);
                        if (sum.empty()) { tg = 2 * d; continue; }   // a cycle no labelling avoids
                        if (sum[0].second < 0) for (std::pair<int, int> &m : sum) m.second = -m.second;
                        std::pair<std::map<Bag, int>::iterator, bool> ins = found.insert(std::make_pair(sum, 2 * d));
                        if (!ins.second && ins.first->second > 2 * d) ins.first->second = 2 * d;
                        if ((long long)found.size() > kMaxEquations) {
                            t.refused_count = (long long)found.size(); t.refused_what = "equations";
                            return false;
                        }
                    }
            layer.swap(next);
        }
    }
    t.tree_girth = tg;
    // the table: walks shorter than what the tree allows, fixed edges dropped, short equations first (they are the cheapest to test)
    std::vector<Bag> rows;
    for (const std::pair<const Bag, int> &f : found) {
        if (f.second >= tg) continue;
        Bag r;
        for (const std::pair<int, int> &m : f.first)
            if (random_index[(size_t)m.first] >= 0) r.push_back(std::make_pair(random_index[(size_t)m.first], m.second));
        if (r.empty()) t.never_accepts = true;
        rows.push_back(r);
    }
    std::stable_sort(rows.begin(), rows.end(), [](const Bag &a, const Bag &b) { return a.size() != b.size() ? a.size() < b.size() : a < b; });
    t.n_equations = (int)rows.size();
    t.eq_begin.assign(1, 0);
    for (const Bag &r : rows) {
        for (const std::pair<int, int> &m : r) { t.term_edge.push_back(m.first); t.term_mult.push_back(m.second); }
        t.eq_begin.push_back((int32_t)t.term_edge.size());
    }
    return true;
}

// the column pairs (j < jc, in upstream's order) whose supports agree: columns that differ in an empty cell are never equal
inline std::vector<int32_t> column_pairs(int rh, int nh, const std::vector<int32_t> &cell) {
    std::vector<int32_t> out;
    for (int j = 0; j < nh; ++j)
        for (int jc = j + 1; jc < nh; ++jc) {
            int i = 0;
            while (i < rh && (cell[(size_t)j * rh + i] == -1) == (cell[(size_t)jc * rh + i] == -1)) ++i;
            if (i == rh) { out.push_back(j); out.push_back(jc); }
        }
    return out;
}

// upstream's check_same_colums on a labelling given per cell (column by column): -1 empty, else the shift
inline bool same_columns(int rh, int nh, const std::vector<int> &by_col) {
    for (int j = 0; j < nh; ++j)
        for (int jc = j + 1; jc < nh; ++jc)
            if (std::equal(by_col.begin() + (size_t)j * rh, by_col.begin() + (size_t)(j + 1) * rh, by_col.begin() + (size_t)jc * rh)) return true;
    return false;
}

}  // namespace ldpc_label

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace ldpc_label {

enum { kRejected = 0, kSurvivors, kAccepted, kEnd, kEvaluated, kChecked, kRedraws, kCounters };   // Args::ctr

struct Args {
    const uint32_t *xw;          // the round's words: xw[i] = raw (untempered) tape word p + i
    uint32_t words;              // words scanned for redraws: n * Er + rej_cap
    uint32_t n;                  // attempts of the round
    long long att_base;          // attempts tested in earlier rounds
    int Er, M;
    uint32_t thresh;             // 2^32 mod M
    uint32_t er_magic;           // floor(2^32 / Er) + 1: j / Er for j < 64 * Er (Er >= 2; one edge needs no division)
    unsigned long long m_magic;  // floor(2^40 / M) + 1: s / M for s < 62 * M, exact as 62 * M * M < 2^40
    uint32_t div_M;              // an attempt dies on a sum divisible by div_M: M; the bank search (ldpc_voltage.hpp) passes 2^22 with
                                 // m_magic = 2^18 + 1, so that s / div_M is 0 for every s < 2^21 and only a zero sum is divisible
    uint32_t *rej_raw, *rej;     // rejected words of the round, as found and ascending
    uint32_t rej_cap;
    int n_eq;
    const int32_t *eq_begin;     // [n_eq + 1]
    const int32_t *terms;        // (edge << 8) | (multiplicity & 0xff)
    unsigned long long *bitmap;  // [ceil(n / 64)] survivors of the equations
    unsigned long long *ctr;     // [kCounters]; kAccepted, kEvaluated and kChecked run over the whole call
    // selection
    int rh, nh, want;
    const int32_t *cell;         // [nh][rh]
    const int32_t *pairs;        // [n_pairs][2] columns j < jc with the same support: the only ones that can be equal
    int n_pairs;
    int16_t *hd_out;             // [want][rh][nh]
    long long *attempt_index;    // [want]
    const int32_t *min_ok_att;   // [n] per attempt of the round, and
    int32_t *min_ok_out;         // [want]: the bank search's smallest lifting; NULL otherwise
    long long p;                 // tape index of xw[0]
    uint32_t *state_next;        // [624] raw words behind the last word drawn
};

__device__ __forceinline__ uint32_t temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

__device__ __forceinline__ uint32_t rejected_count(const Args &a) {
    const unsigned long long c = a.ctr[kRejected];
    return c < a.rej_cap ? (uint32_t)c : a.rej_cap;
}

// round-local word index of draw j: j plus the redraws in front of it (R[k] - k draws precede rejected word R[k])
__device__ __forceinline__ uint32_t word_of_draw(const Args &a, uint32_t nrej, uint32_t j) {
    uint32_t lo = 0, hi = nrej;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.rej[mid] - mid <= j) lo = mid + 1; else hi = mid;
    }
    return j + lo;
}

// rejected words in front of word i
__device__ __forceinline__ uint32_t redraws_before(const Args &a, uint32_t nrej, uint32_t i) {
    uint32_t lo = 0, hi = nrej;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.rej[mid] < i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) mark_kernel(const Args a) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.words; i += stride) {
        const uint32_t low = temper(a.xw[i]) * (uint32_t)a.M;
        if (low < a.thresh) {
            const unsigned long long k = atomicAdd(&a.ctr[kRejected], 1ull);
            if (k < a.rej_cap) a.rej_raw[k] = i;
        }
    }
}

// the positions are distinct: the rank of one is the number of smaller ones
__global__ void __launch_bounds__(256) sort_kernel(const Args a) {
    const uint32_t n = rejected_count(a);
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint32_t v = a.rej_raw[i];
        uint32_t rank = 0;
        for (uint32_t k = 0; k < n; ++k) rank += a.rej_raw[k] < v ? 1u : 0u;
        a.rej[rank] = v;
    }
}

// the shifts of attempts att0 .. att0 + 63 (those below a.n) -> v[edge * kRowStride + attempt]; the T threads read the words coalesced,
// four loads in flight per thread (a lone workgroup, as in select_kernel, would otherwise wait for every word in turn)
template <int T>
__device__ __forceinline__ void load_shifts(const Args &a, uint32_t nrej, uint32_t att0, int16_t *v, int tid) {
    const uint32_t natt = a.n - att0 < 64u ? a.n - att0 : 64u;
    const uint32_t j0 = att0 * (uint32_t)a.Er, j1 = j0 + natt * (uint32_t)a.Er;
    const uint32_t w0 = word_of_draw(a, nrej, j0), w1 = word_of_draw(a, nrej, j1 - 1) + 1;
    for (uint32_t i0 = w0 + tid; i0 < w1; i0 += 4 * T) {
        uint32_t raw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) raw[u] = i0 + u * T < w1 ? a.xw[i0 + u * T] : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + u * T;
            const unsigned long long prod = (unsigned long long)temper(raw[u]) * (uint32_t)a.M;
            if (i >= w1 || (uint32_t)prod < a.thresh) continue;
            const uint32_t j = i - (nrej ? redraws_before(a, nrej, i) : 0u) - j0;   // draw of the wave, < 64 * Er
            const uint32_t att = a.Er == 1 ? j : __umulhi(j, a.er_magic), e = j - att * (uint32_t)a.Er;
            if (att < 64u) v[e * kRowStride + att] = (int16_t)(prod >> 32);   // always, unless the redraw list overflowed (the host fails the call then)
        }
    }
}

__global__ void __launch_bounds__(64) check_kernel(const Args a) {
    extern __shared__ int16_t label_v[];
    const int lane = threadIdx.x;
    const uint32_t att0 = blockIdx.x * 64u;
    const uint32_t nrej = rejected_count(a);
    load_shifts<64>(a, nrej, att0, label_v, lane);
    __syncthreads();
    bool alive = att0 + lane < a.n;
    uint32_t evaluated = 0;
    const int16_t *mine = label_v + lane;
    for (int eq = 0; eq < a.n_eq; ++eq) {
        if (__ballot(alive) == 0ull) break;
        const int b = a.eq_begin[eq], e = a.eq_begin[eq + 1];
        int sum = 0;
        for (int t = b; t < e; ++t) {
            const int w = a.terms[t];
            sum += (int)(int8_t)(w & 0xff) * (int)mine[(w >> 8) * kRowStride];
        }
        const uint32_t s = (uint32_t)(sum < 0 ? -sum : sum);
        const uint32_t q = (uint32_t)(((unsigned long long)s * a.m_magic) >> 40);
        evaluated += alive ? 1u : 0u;
        alive = alive && s != q * a.div_M;
    }
    const unsigned long long mask = __ballot(alive);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) evaluated += __shfl_xor(evaluated, o);
    if (lane == 0) {
        a.bitmap[blockIdx.x] = mask;
        if (mask) atomicAdd(&a.ctr[kSurvivors], (unsigned long long)__popcll(mask));
        atomicAdd(&a.ctr[kEvaluated], (unsigned long long)evaluated);
    }
}

__device__ __forceinline__ int cell_value(const int32_t c, const int16_t *mine) { return c == -1 ? -1 : c == -2 ? 0 : (int)mine[c * kRowStride]; }

// one workgroup: the survivors in attempt order, upstream's equal-columns test, the first labellings that pass, the generator's
// position.  Its first wave holds one attempt per lane, as check_kernel does; all four waves load the shifts and write the results.
constexpr int kSelectThreads = 256;

__global__ void __launch_bounds__(kSelectThreads) select_kernel(const Args a) {
    extern __shared__ int16_t label_v[];
    __shared__ long long s_end;
    __shared__ unsigned long long s_okm;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t nrej = rejected_count(a);
    const uint32_t nw = (a.n + 63u) / 64u;
    const int cells = a.rh * a.nh;
    long long have = (long long)a.ctr[kAccepted];
    long long end = -1;
    const int16_t *mine = label_v + lane;
    if (a.ctr[kSurvivors] != 0ull)
        for (uint32_t base = 0; base < nw && have < a.want; base += 64) {
            unsigned long long any = __ballot(base + lane < nw && a.bitmap[base + lane] != 0ull);   // the same in every wave
            while (any && have < a.want) {
                const uint32_t wave = base + (uint32_t)(__ffsll((long long)any) - 1);
                any &= any - 1ull;
                const unsigned long long mask = a.bitmap[wave];
                __syncthreads();   // the shifts of the wave before have been read
                load_shifts<kSelectThreads>(a, nrej, wave * 64u, label_v, tid);
                __syncthreads();
                if (tid < 64) {
                    bool ok = (mask >> lane) & 1ull;
                    if (ok) {
                        bool same = false;
                        for (int q = 0; q < a.n_pairs && !same; ++q) {
                            const int j = a.pairs[2 * q], jc = a.pairs[2 * q + 1];
                            int i = 0;
                            while (i < a.rh && cell_value(a.cell[j * a.rh + i], mine) == cell_value(a.cell[jc * a.rh + i], mine)) ++i;
                            same = i == a.rh;
                        }
                        ok = !same;
                    }
                    const unsigned long long okm = __ballot(ok);
                    if (tid == 0) s_okm = okm;
                }
                __syncthreads();
                unsigned long long okm = s_okm;
                const long long got = __popcll(okm);
                for (long long k = have; okm && k < a.want; ++k) {   // the labellings that pass, in attempt order
                    const int l = __ffsll((long long)okm) - 1;
                    okm &= okm - 1ull;
                    int16_t *out = a.hd_out + (size_t)k * cells;
                    for (int c = tid; c < cells; c += kSelectThreads) {   // c counts column by column, as the cells do
                        const int j = c / a.rh, i = c - j * a.rh;
                        out[i * a.nh + j] = (int16_t)cell_value(a.cell[c], label_v + l);
                    }
                    if (tid == 0) {
                        const uint32_t att = wave * 64u + (uint32_t)l;
                        a.attempt_index[k] = a.att_base + att;
                        if (a.min_ok_out) a.min_ok_out[k] = a.min_ok_att[att];
                        if (k == a.want - 1) s_end = a.p + word_of_draw(a, nrej, (att + 1u) * (uint32_t)a.Er - 1u) + 1;
                    }
                }
                have += got;
            }
        }
    __syncthreads();
    if (have >= a.want) {
        have = a.want;
        end = s_end;   // written with the last labelling, before the barrier above
    } else {
        end = a.p + word_of_draw(a, nrej, a.n * (uint32_t)a.Er - 1u) + 1;   // every attempt of the round was drawn
    }
    for (int i = tid; i < 624; i += kSelectThreads) a.state_next[i] = a.xw[end - a.p + i];
    if (tid == 0) {
        a.ctr[kAccepted] = (unsigned long long)have;
        a.ctr[kEnd] = (unsigned long long)end;
        a.ctr[kChecked] += a.n;
        a.ctr[kRedraws] += redraws_before(a, nrej, (uint32_t)(end - a.p));
    }
}

}  // namespace ldpc_label
#endif  // __HIPCC__
