// K6: fused sampler — greedy / temperature / top-k / top-p, graph-safe RNG — and, in the
// captured decode step, the step's bookkeeping, in ONE launch (r02: six sampler launches +
// decode_advance = 47 us per step, profiles/r03/prof8.md).
//
// Sampling is Gumbel-max: token = argmax(z_i + g_i) over the allowed set, z = (logit - max)/T,
// g_i = -log(-log(u_i)), u_i a counter-based hash of (seed, offset, i): no RNG state, so a
// captured hipGraph replays deterministically and a knight's stream depends only on
// (seed, knight, position) (the engine passes each row's token position as `offset`).
//
// Grid (B, C): C workgroups per row stream one chunk each and publish, write-through,
//   chunk_records       the chunk's max / argmax / min and its best Gumbel score over ALL its tokens,
//   publish_chunk_hist  (top-p rows) the chunk's mass per bin of a grid aligned across chunks,
//   publish_chunk_topk  (top-k rows, k <= KMAX) the chunk's own top-k tokens,
// then take_ticket; the row's LAST-arriving workgroup (the "decider", MI355X_MICROARCH sc1 hand-off
// table row 1) fetches everything in one round trip (load_row_records) and finishes the row alone:
//   * greedy / unfiltered rows: the reduced chunk records decide (smp_kernel itself);
//   * top-p rows, accept_test: j* = argmax(z + g) over the whole vocabulary is the nucleus sample
//     whenever the mass of the tokens strictly more likely than j* is below p * total (then the
//     argmax over the nucleus is j*); j* is itself a softmax draw, so that holds with probability
//     >= top_p. The chunk histograms bound both masses; one exact pass over the row when j*
//     shares a bin with the cut;
//   * a rejected j*: nucleus_from_chunk_hists (the cut from the same histograms, a rescan of the
//     chunks whose best token is outside), else nucleus_by_candidates (the chunks' bests in score
//     order, one pass for the mass above each);
//   * top-k rows with lists: topk_from_lists (plain top-k, and top-p inside the top-k set);
//   * otherwise: threshold_by_histogram — a 2048-bin histogram of z in LDS (count + mass) -> the
//     crossing bin -> a 2048-bin sub-histogram of that bin -> threshold (coarse bins over the
//     row's own z range, at most [-ZR, 0]; resolution range / 4M <= 7e-6 in z) — and
//     argmax_allowed, the Gumbel argmax over the allowed set.
// finish_row then writes the token and, with bookkeeping on (sample_advance), the decode_advance
// + decode_prep work of its row (out[step, b], ids, positions, lengths, next K/V slot, sampler
// offset, embedding row); the last decider of the launch bumps `step`. Every counter re-arms
// itself, so the workspace is zeroed once (ops.sample_workspace) and replays need no memset.
// Nothing here spins: a workgroup that is not the decider returns after its ticket.
// Bit-for-bit RNG twin: theroundtaible_amd/ops/reference.py::uniform_tensor.
#include "sampling_prims.h"
#include "step_core.h"

#include <cstdlib>

namespace {
using namespace smp;
constexpr int C = 32;       // chunks (workgroups) per row
constexpr float ZR = 30.f;  // exp(-30) * 128K < 1e-8 of the mass: ignored

// per-row workspace (4-byte words, floats / ints interchangeable)
constexpr int W_MAX = 0;                 // [C] chunk max
constexpr int W_ARG = W_MAX + C;         // [C] chunk argmax (int)
constexpr int W_GV = W_ARG + C;          // [C] chunk best Gumbel score v/T + g
constexpr int W_GI = W_GV + C;           // [C] its token (int)
constexpr int W_MIN = W_GI + C;          // [C] chunk min
constexpr int W_CNT = W_MIN + C;         // arrival ticket (int), re-armed by the decider
constexpr int W_SC = W_CNT + 1;          // histogram grid scale for the next launch (float, 0 = default)
constexpr int W_KB = W_CNT + 4;          // [C] chunk's top histogram bin floor(max * scale) (int)
constexpr int HB = 128;                  // histogram bins per chunk (the last one: everything lower)
constexpr float BW = 16.f;               // bins per unit of z = logit / T
constexpr int W_HIST = W_KB + C;         // [C][HB] chunk mass per bin, relative to the chunk max
// top-k rows with k <= KMAX: every chunk publishes its own top-k tokens (ties at its k-th key
// included up to LCAP), sorted by token id; the decider merges the C lists
constexpr int KMAX = 64;
constexpr int LCAP = 96;
constexpr int W_TKN = W_HIST + C * HB;   // [C] list length | truncated << 16 (int)
constexpr int W_TKK = W_TKN + C;         // [C] the chunk's k-th largest order key (int)
constexpr int W_TKL = W_TKK + C;         // [C][LCAP] order keys (int)
constexpr int W_TKI = W_TKL + C * LCAP;  // [C][LCAP] token ids (int)
constexpr int W_ROW = W_TKI + C * LCAP;  // words per row; after the B rows: the rows-done ticket
// LDS pool: the decider's histograms or, on top-k list rows, the chunk's order keys (chunk
// phase) / the merged lists and the allowed set (decider); see Smem
constexpr int POOL_BYTES = NB * 4 * 3 + NB * 8;
constexpr int POOLK = POOL_BYTES / 4;
constexpr int NALLOW = NT;               // list path: at most this many allowed tokens (else the histogram path)
constexpr int HVQ = C * HB / NT;         // chunk histogram words per decider thread
constexpr int NC = 4;                    // candidates per mass-above pass (nucleus_by_candidates)
// which branch decided a row (RT_SMP_PROBE=5 writes it in place of the token; + PATH_EXACT_PASS
// when the accept test needed its exact pass over the row)
constexpr int PATH_PLAIN = 0, PATH_ACCEPT = 1, PATH_RESCAN = 2, PATH_CANDIDATES = 3, PATH_HISTOGRAM = 4,
              PATH_EXACT_PASS = 10;

// the 16-byte vector of a row's elements
template <typename T> struct RowVec;
template <> struct RowVec<uint16_t> {
  using type = rt::short8;
  static RT_DEVICE float get(const type& v, int j) { return rt::bf2f((uint16_t)v[j]); }
};
template <> struct RowVec<float> {
  using type = rt::float4_;
  static RT_DEVICE float get(const type& v, int j) { return v[j]; }
};

// f(i, v) over [lo, hi) of a row, NT-strided: 16-byte loads when the row is aligned (VEC; lo % 8
// == 0), then a scalar tail. `first`, when given, is this thread's first vector of the range,
// loaded by the caller (whatever it holds when the range has no vector for this thread). UNR =
// the 16-byte loads a lane keeps in flight before consuming them: the decider's whole-row passes
// stream 256 KB on ONE CU and take 8 (a load-use loop would pay one memory round trip per 16
// bytes per lane); a chunk is at most two vectors per lane and takes 1. fp32 rows load one
// vector at a time whatever UNR says (the served logits are bf16).
template <typename T, bool VEC, int UNR, typename F>
RT_DEVICE void sweep(const T* row, int lo, int hi, F&& f, const typename RowVec<T>::type* first = nullptr) {
  int tail = lo;
  if constexpr (VEC) {
    using VT = typename RowVec<T>::type;
    constexpr int SH = sizeof(T) == 2 ? 3 : 2, N = 1 << SH, U = sizeof(T) == 2 ? UNR : 1;
    const int nv = (hi - lo) >> SH;
    const VT* p = reinterpret_cast<const VT*>(row + lo);
    auto eat = [&](int c, const VT& v) {
#pragma unroll
      for (int j = 0; j < N; ++j) f(lo + c * N + j, RowVec<T>::get(v, j));
    };
    int c = threadIdx.x;
    if (first != nullptr) {
      if (c < nv) eat(c, *first);
      c += NT;
    }
    if constexpr (U > 1) {
      for (; c + (U - 1) * NT < nv; c += U * NT) {
        VT v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = p[c + u * NT];
#pragma unroll
        for (int u = 0; u < U; ++u) eat(c + u * NT, v[u]);
      }
    }
    for (; c < nv; c += NT) eat(c, p[c]);
    tail = lo + (nv << SH);
  }
  for (int i = tail + threadIdx.x; i < hi; i += NT) f(i, rt::DT<T>::load(row + i));
}
constexpr int ROW_UNR = 8;   // whole-row passes

RT_DEVICE void chunk_range(int V, int c, int& lo, int& hi) {
  const int per = ((V + C - 1) / C + 7) & ~7;
  lo = min(V, c * per);
  hi = min(V, lo + per);
}

// histogram mass in 32.32 fixed point: the accumulators are INTEGER LDS atomics (count, and mass)
// — LDS float atomic adds serialize per lane on gfx950 (r03 probe: a 128K-token coarse pass took
// 320 us on one workgroup), the integer ones do not
RT_DEVICE unsigned long long mass_fixed(float m) { return (unsigned long long)(m * 4294967296.f); }
RT_DEVICE float mass_float(unsigned long long m) { return (float)(m >> 8) * (1.f / 16777216.f); }

// All of the workgroup's LDS, declared once in the kernel. `pool` is overlaid, one use at a time:
//   histograms (decider)            counts() / mass() as floats, counts_acc() / mass_acc() their
//                                   integer accumulators (chunk phase: mass_acc()[HB] only);
//   order keys (chunk, list rows)   order_keys()[hi - lo];
//   merged lists (decider)          merged_keys() / merged_ids() [C][LCAP], then the allowed set
//                                   allow_keys() / allow_ids() / allow_mass() [NALLOW] in id order.
// The arrays come first, each a multiple of 16 bytes, so every one starts 16-byte aligned as a
// __shared__ array of its own would (every thread reads the NWV per-wave words of a reduction as
// 16-byte LDS loads); `red` and the single words follow.
struct Smem {
  unsigned char pool[POOL_BYTES] __attribute__((aligned(16)));
  // scratch of the block reductions, kth_key and first_crossing
  float sv[NWV];
  int si[NWV], cnt3[2 * 3 * NWV];
  // chunk phase: the list under construction (keys above the chunk's k-th, then its ties)
  uint32_t list_k[LCAP], tie_k[LCAP];
  int list_i[LCAP], tie_i[LCAP];
  // decider: what the C chunks published
  float cmax[C], cgv[C], cmin[C], csc[C];
  int carg[C], cgi[C], ckb[C], tkn[C], tkk[C];
  // decider: path-local arrays
  int rescan_flag[C];                    // nucleus_from_chunk_hists
  int ord[C], ui[NC];                    // nucleus_by_candidates
  float cv[NC], uv[NC], us[NC];
  int ccnt[C];                           // topk_from_lists
  int rescan_list[C];                    // argmax_allowed
  float red[2 * NWV + 2];
  // single words: first_crossing's result and prefixes, the list lengths, "this workgroup took the
  // row's last ticket", and one word each of the four paths above
  int res;
  float pa, pb;
  int list_n, tie_n, last, lump, flag, fallback, nres;

  RT_DEVICE float* counts() { return reinterpret_cast<float*>(pool); }
  RT_DEVICE float* mass() { return counts() + NB; }
  RT_DEVICE unsigned* counts_acc() { return reinterpret_cast<unsigned*>(mass() + NB); }
  RT_DEVICE unsigned long long* mass_acc() { return reinterpret_cast<unsigned long long*>(counts_acc() + NB); }
  RT_DEVICE uint32_t* order_keys() { return reinterpret_cast<uint32_t*>(pool); }
  RT_DEVICE uint32_t* merged_keys() { return order_keys(); }
  RT_DEVICE int* merged_ids() { return reinterpret_cast<int*>(order_keys() + C * LCAP); }
  RT_DEVICE uint32_t* allow_keys() { return order_keys() + 2 * C * LCAP; }
  RT_DEVICE int* allow_ids() { return reinterpret_cast<int*>(allow_keys() + NALLOW); }
  RT_DEVICE float* allow_mass() { return reinterpret_cast<float*>(allow_ids() + NALLOW); }

  // zero the first n bins' accumulators (COUNTS: the counts too), then a barrier
  template <bool COUNTS>
  RT_DEVICE void hist_clear(int n = NB) {
    for (int i = threadIdx.x; i < n; i += NT) {
      if constexpr (COUNTS) counts_acc()[i] = 0u;
      mass_acc()[i] = 0ull;
    }
    __syncthreads();
  }
  // barrier, accumulators -> counts() / mass() (no COUNTS: counts() = 0), barrier
  template <bool COUNTS>
  RT_DEVICE void hist_to_float() {
    __syncthreads();
    for (int i = threadIdx.x; i < NB; i += NT) {
      counts()[i] = COUNTS ? (float)counts_acc()[i] : 0.f;
      mass()[i] = mass_float(mass_acc()[i]);
    }
    __syncthreads();
  }
};
static_assert(2 * C * LCAP + 3 * NALLOW <= POOLK, "merged lists + allowed set fit the pool");

constexpr float NEVER = 3.0e38f;   // a first_crossing target that no prefix reaches
// first bin of the current histogram whose count prefix reaches `count` / mass prefix reaches `m`
RT_DEVICE int crossing(Smem& sm, float count, float m) {
  return first_crossing(sm.counts(), sm.mass(), count, m, sm.red, &sm.res, &sm.pa, &sm.pb);
}

struct SampleArgs {
  int64_t* tok;                 // [B] sampled ids
  float* ws;                    // B * W_ROW + 4 words, zero before the first launch (self re-arming)
  const void* logits;
  int V;
  int64_t ld;
  const float* temperature;
  const float* top_p;
  const int* top_k;
  const int64_t* seeds;
  const int64_t* offsets;       // read by every workgroup; with prep, prep.offsets is the same vector
  int B;
  // decode-step bookkeeping (adv = 1): decode_advance + next-step decode_prep of each row
  int adv;
  int64_t* out;                 // [max_steps, B]
  int64_t* ids;
  int64_t* positions;
  int* ctx_lens;
  int64_t* step;
  int max_steps;
  rt::PrepArgs prep;            // all null: no prep
  int probe;                    // RT_SMP_PROBE=5 (tools/probes): tok[b] = the path that decided (PATH_*)
};

// The constants of this workgroup's row, built once after the single wait for the parameter loads.
template <typename T>
struct RowConst {
  static constexpr int KLO = sizeof(T) == 2 ? 16 : 0;   // order keys: bits below KLO carry no order
  const T* ptr;
  float* w;        // the row's workspace words, as floats and as ints
  int* wi;
  int row, V;
  float temp, invT;
  uint64_t key;    // RNG key of (seed, offset)
  float p;
  int k;
  bool use_k;      // top-k filters: 0 < k < V
  bool hist;       // top-p rows (no top-k): every chunk publishes a mass histogram
  bool lst;        // top-k rows with a small k: every chunk publishes its top-k list
  float sbin;      // histogram grid: bins per logit unit
};
template <typename T>
RT_DEVICE RowConst<T> row_constants(const SampleArgs& a, int b, float temp, int64_t off, float sgrid, int k, float p) {
  RowConst<T> r;
  r.ptr = static_cast<const T*>(a.logits) + (size_t)b * a.ld;
  r.w = a.ws + (size_t)b * W_ROW;
  r.wi = reinterpret_cast<int*>(r.w);
  r.row = b;
  r.V = a.V;
  r.temp = temp;
  r.invT = temp > 0.f ? 1.f / temp : 0.f;
  r.key = mix64((uint64_t)a.seeds[b] ^ mix64((uint64_t)off));
  r.p = p;
  r.k = k;
  r.use_k = k > 0 && k < a.V;
  // top-p rows (no top-k): every chunk also publishes a histogram of its tokens' mass on a grid
  // aligned across chunks (bin = floor(logit * scale)), which decides the accept test without
  // another pass over the row for all but the rows whose j* shares a bin with the cut
  r.hist = temp > 0.f && p < 1.f && !r.use_k;
  // grid scale: chosen by the previous launch's decider from the row's value span (0 before the
  // first launch: the default)
  r.sbin = sgrid > 0.f ? sgrid : r.invT * BW;
  // top-k rows with a small k: chunk top-k lists (the decider needs no pass over the row)
  const int per = ((a.V + C - 1) / C + 7) & ~7;
  r.lst = temp > 0.f && r.use_k && k <= KMAX && per <= POOLK;
  return r;
}
template <typename T>
RT_DEVICE bool in_row(const RowConst<T>& r, int i) {
  return i >= 0 && i < r.V;
}

// relaxed agent-scope publication / fetch of one workspace word
template <typename W>
RT_DEVICE void publish(W* p, W v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename W>
RT_DEVICE W fetch(const W* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- chunk phases (every workgroup) ----

struct ChunkRec {
  ArgMax am, gb;   // max / argmax of the chunk's values; best Gumbel score v/T + g and its token
  float mn;
};
// One sweep of the chunk [lo, hi): max, argmax, min and the best Gumbel score over ALL its tokens
// (greedy rows: max / argmax only); list rows also leave every token's order key in
// sm.order_keys()[i - lo].
template <typename T, bool VEC>
RT_DEVICE ChunkRec chunk_records(const RowConst<T>& r, int lo, int hi, const typename RowVec<T>::type* first,
                                 Smem& sm) {
  ChunkRec rec{{-INFINITY, NO_TOKEN}, {-INFINITY, NO_TOKEN}, INFINITY};
  if (r.temp > 0.f) {
    uint32_t* okeys = sm.order_keys();
    sweep<T, VEC, 1>(r.ptr, lo, hi, [&](int i, float v) {
      am_merge(rec.am, v, i);
      rec.mn = fminf(rec.mn, v);
      am_merge(rec.gb, v * r.invT + gumbel(r.key, (uint32_t)i), i);
      if (r.lst) okeys[i - lo] = okey(v, r.KLO);
    }, first);
    rec.gb = block_argmax(rec.gb, sm.sv, sm.si);
    rec.mn = -block_reduce<Max>(-rec.mn, sm.red);
  } else {
    sweep<T, VEC, 1>(r.ptr, lo, hi, [&](int i, float v) { am_merge(rec.am, v, i); }, first);
  }
  rec.am = block_argmax(rec.am, sm.sv, sm.si);
  return rec;
}

// Top-p rows: a second sweep of the (L2-resident) chunk sums the mass exp((v - chunk max) / T)
// per grid bin below the chunk's top bin, and publishes the HB bins and the top bin's index.
// Every thread's stores have completed when this returns (the ticket follows).
template <typename T, bool VEC>
RT_DEVICE void publish_chunk_hist(const RowConst<T>& r, int c, int lo, int hi,
                                  const typename RowVec<T>::type* first, float cmax, Smem& sm) {
  const float ktop = floorf(cmax * r.sbin);
  unsigned long long* hmi = sm.mass_acc();
  sm.hist_clear<false>(HB);
  if (cmax > -INFINITY) {
    sweep<T, VEC, 1>(r.ptr, lo, hi, [&](int, float v) {
      const float e = __expf((v - cmax) * r.invT);
      if (e > 0.f) {
        const float kr = fminf(fmaxf(ktop - floorf(v * r.sbin), 0.f), (float)(HB - 1));
        atomicAdd(&hmi[(int)kr], mass_fixed(e));
      }
    }, first);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < HB; i += NT) publish(&r.w[W_HIST + c * HB + i], mass_float(hmi[i]));
  if (threadIdx.x == 0) publish(&r.wi[W_KB + c], cmax > -INFINITY ? (int)ktop : -(1 << 30));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // every thread's histogram stores complete before thread 0's ticket
}

// Top-k list rows: this chunk's k-th largest key Kc (from the order keys chunk_records left);
// list = every token above it, then its ties up to LCAP, published sorted by token id (the
// atomic slot order is not deterministic) with its length (| truncated << 16) and Kc. Every
// thread's stores have completed when this returns (the ticket follows).
template <typename T>
RT_DEVICE void publish_chunk_topk(const RowConst<T>& r, int c, int lo, int hi, Smem& sm) {
  const uint32_t* okeys = sm.order_keys();
  const int n = hi - lo;
  const int need = min(r.k, n);
  uint32_t kc = 0;
  if (need > 0) kc = kth_key(okeys, n, need, r.KLO, sm.cnt3);
  if (threadIdx.x == 0) sm.list_n = sm.tie_n = 0;
  __syncthreads();
  if (need > 0) {   // one pass: keys above kc (fewer than need <= KMAX < LCAP) and ties apart
    for (int i0 = 0; i0 < n; i0 += 8 * NT) {
      uint32_t kk[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + (int)threadIdx.x + j * NT;
        kk[j] = i < n ? okeys[i] : 0u;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + (int)threadIdx.x + j * NT;
        if (kk[j] > kc) {   // fewer than need <= KMAX < LCAP such keys; bounded all the same
          const int sl = atomicAdd(&sm.list_n, 1);
          if (sl < LCAP) {
            sm.list_k[sl] = kk[j];
            sm.list_i[sl] = lo + i;
          }
        } else if (kk[j] == kc && i < n) {
          const int sl = atomicAdd(&sm.tie_n, 1);
          if (sl < LCAP) {
            sm.tie_k[sl] = kk[j];
            sm.tie_i[sl] = lo + i;
          }
        }
      }
    }
    __syncthreads();
    const int g = sm.list_n;
    for (int q = threadIdx.x; q < min(sm.tie_n, LCAP - g); q += NT) {
      sm.list_k[g + q] = sm.tie_k[q];
      sm.list_i[g + q] = sm.tie_i[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) sm.list_n = g + sm.tie_n;
  }
  __syncthreads();
  const int len = min(sm.list_n, LCAP);
  if ((int)threadIdx.x < len) {
    const int mi = sm.list_i[threadIdx.x];
    int rank = 0;
    for (int j = 0; j < len; ++j) rank += sm.list_i[j] < mi;
    publish(&r.wi[W_TKL + c * LCAP + rank], (int)sm.list_k[threadIdx.x]);
    publish(&r.wi[W_TKI + c * LCAP + rank], mi);
  }
  if (threadIdx.x == 0) {
    publish(&r.wi[W_TKN + c], len | (sm.list_n > LCAP ? 1 << 16 : 0));
    publish(&r.wi[W_TKK + c], (int)kc);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // every thread's list stores complete before thread 0's ticket
}

// Thread 0 publishes the chunk record, waits for those stores, and takes the row's ticket; the
// last of the C arrivals re-arms it. Returns whether this workgroup is the row's decider.
template <typename T>
RT_DEVICE bool take_ticket(const RowConst<T>& r, int c, const ChunkRec& rec, Smem& sm) {
  if (threadIdx.x == 0) {
    publish(&r.w[W_MIN + c], rec.mn);
    publish(&r.w[W_MAX + c], rec.am.v);
    publish(&r.wi[W_ARG + c], rec.am.i);
    publish(&r.w[W_GV + c], rec.gb.v);
    publish(&r.wi[W_GI + c], rec.gb.i);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int prev = __hip_atomic_fetch_add(&r.wi[W_CNT], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sm.last = prev == C - 1;
    if (sm.last) publish(&r.wi[W_CNT], 0);
  }
  __syncthreads();
  return sm.last;
}

// ---- the decider ----

struct RowRec {
  ArgMax ra, g;   // the row's max / argmax; j* = its best Gumbel score over ALL tokens
  float rmin;
};
// ONE round trip for everything the chunks published: the records into sm.c*, on top-p rows the
// grid tops and the 4096 histogram words (HVQ per thread, into hv), on list rows the C lists
// (6 + 6 words per thread) into sm.merged_keys() / merged_ids(), entries past a chunk's length
// with key 0 (below every value's key). Returns the reduced records.
template <typename T>
RT_DEVICE RowRec load_row_records(const RowConst<T>& r, Smem& sm, float (&hv)[HVQ]) {
  const float* w = r.w;
  const int* wi = r.wi;
  if (threadIdx.x < C) {
    const int j = threadIdx.x;
    sm.cmax[j] = fetch(&w[W_MAX + j]);
    sm.carg[j] = fetch(&wi[W_ARG + j]);
    sm.cgv[j] = fetch(&w[W_GV + j]);
    sm.cgi[j] = fetch(&wi[W_GI + j]);
    sm.cmin[j] = fetch(&w[W_MIN + j]);
    if (r.hist) sm.ckb[j] = fetch(&wi[W_KB + j]);
  }
  if (r.hist) {
#pragma unroll
    for (int q = 0; q < HVQ; ++q) hv[q] = fetch(&w[W_HIST + threadIdx.x + q * NT]);
  }
  if (r.lst) {
    constexpr int LQ = C * LCAP / NT;
    int lkr[LQ], lir[LQ];
    if (threadIdx.x < C) {
      sm.tkn[threadIdx.x] = fetch(&wi[W_TKN + threadIdx.x]);
      sm.tkk[threadIdx.x] = fetch(&wi[W_TKK + threadIdx.x]);
    }
#pragma unroll
    for (int q = 0; q < LQ; ++q) {
      lkr[q] = fetch(&wi[W_TKL + threadIdx.x + q * NT]);
      lir[q] = fetch(&wi[W_TKI + threadIdx.x + q * NT]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LQ; ++q) {
      const int e = threadIdx.x + q * NT, cc = e / LCAP;
      sm.merged_keys()[e] = e - cc * LCAP < (sm.tkn[cc] & 0xffff) ? (uint32_t)lkr[q] : 0u;
      sm.merged_ids()[e] = lir[q];
    }
  }
  __syncthreads();
  RowRec d{{-INFINITY, NO_TOKEN}, {-INFINITY, NO_TOKEN}, INFINITY};
  for (int j = 0; j < C; ++j) {
    am_merge(d.ra, sm.cmax[j], sm.carg[j]);
    am_merge(d.g, sm.cgv[j], sm.cgi[j]);
    d.rmin = fminf(d.rmin, sm.cmin[j]);
  }
  return d;
}

struct Accept {
  bool accepted;   // j* is inside the nucleus
  bool decided;    // ... by the histogram bounds alone (no pass over the row)
  float pz;        // p * total mass, the cut (relative to the row max)
  float vj;        // j*'s logit
};
// Top-p fast path: is j* inside the nucleus, i.e. is the mass strictly above it below p * total?
// Bounds on that mass from the chunk histograms (hv): bins above j*'s bin are above it, its own
// bin (and a chunk's open-ended last bin reaching it) may or may not be. When j* shares its bin
// with the cut: the exact test, one pass over the row. Leaves sm.csc = each chunk's scale
// exp((chunk max - row max) / T) for nucleus_from_chunk_hists.
template <typename T, bool VEC>
RT_DEVICE Accept accept_test(const RowConst<T>& r, const RowRec& d, const float (&hv)[HVQ], Smem& sm) {
  const float mx = d.ra.v;
  Accept t;
  t.vj = rt::DT<T>::load(r.ptr + d.g.i);
  const float kj = floorf(t.vj * r.sbin);
  float lo_m = 0.f, mid_m = 0.f, tot_m = 0.f;
  if (threadIdx.x < C) sm.csc[threadIdx.x] = __expf((sm.cmax[threadIdx.x] - mx) * r.invT);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < HVQ; ++q) {
    const int e = threadIdx.x + q * NT, cc = e / HB, kk = e - cc * HB;
    const float m = hv[q] * sm.csc[cc];
    const float kb = (float)(sm.ckb[cc] - kk);   // this bin's grid index (the last bin: its top)
    tot_m += m;
    if (kk < HB - 1) {
      lo_m += kb > kj ? m : 0.f;
      mid_m += kb == kj ? m : 0.f;
    } else {
      mid_m += kb >= kj ? m : 0.f;
    }
  }
  lo_m = block_reduce<Sum>(lo_m, sm.red);
  mid_m = block_reduce<Sum>(mid_m, sm.red);
  tot_m = block_reduce<Sum>(tot_m, sm.red);
  t.pz = r.p * tot_m;
  t.decided = lo_m + mid_m < t.pz || lo_m >= t.pz;
  t.accepted = lo_m + mid_m < t.pz;
  if (!t.decided) {
    const float vj = t.vj;
    float above = 0.f, total = 0.f;
    sweep<T, VEC, ROW_UNR>(r.ptr, 0, r.V, [&](int, float v) {
      const float e = __expf((v - mx) * r.invT);
      total += e;
      above += v > vj ? e : 0.f;
    });
    above = block_reduce<Sum>(above, sm.red);
    total = block_reduce<Sum>(total, sm.red);
    t.pz = r.p * total;
    t.accepted = above < t.pz;
  }
  return t;
}

// Rejected j*: the nucleus cut from the SAME chunk histograms, merged on the common z grid
// (bin g = kmax - floor(v / T * BW), 0 = top). With the crossing bin g*, tokens in bins above it
// are inside the nucleus, below it outside, in it undecided. A chunk's best Gumbel token inside
// the nucleus is its best allowed one; chunks whose best is not are rescanned (tokens above g*
// only). Exact unless an undecided token (bin g*, or an open-ended last bin reaching g*) could
// win: then -1, and the candidate / histogram paths decide. Needs sm.csc from accept_test.
template <typename T, bool VEC>
RT_DEVICE int nucleus_from_chunk_hists(const RowConst<T>& r, float pz, Smem& sm) {
  int kmx = -(1 << 30);
  for (int j = 0; j < C; ++j) kmx = max(kmx, sm.ckb[j]);
  if (threadIdx.x == 0) sm.lump = NB;
  sm.hist_clear<false>();
  for (int q = 0; q < HVQ; ++q) {   // re-read (L2): the registers of accept_test are not kept live across the passes
    const int e = threadIdx.x + q * NT, cc = e / HB, kk = e - cc * HB;
    const float m = fetch(&r.w[W_HIST + e]) * sm.csc[cc];
    const int gb = kmx - (sm.ckb[cc] - kk);
    if (m > 0.f) {
      if (kk == HB - 1 || gb >= NB) atomicMin(&sm.lump, min(gb, NB - 1));   // open-ended: its top
      else atomicAdd(&sm.mass_acc()[gb], mass_fixed(m));
    }
  }
  sm.hist_to_float<false>();
  const int gst = crossing(sm, NEVER, pz);
  if (!(gst < NB && sm.lump > gst)) return -1;
  if (threadIdx.x < C) {
    const int j = threadIdx.x, gi = sm.cgi[j];
    const int gb = in_row(r, gi) ? kmx - (int)floorf(rt::DT<T>::load(r.ptr + gi) * r.sbin) : NB;
    sm.rescan_flag[j] = gb < gst ? 0 : 1;
  }
  __syncthreads();
  ArgMax win{-INFINITY, NO_TOKEN}, amb{-INFINITY, NO_TOKEN};
  for (int j = 0; j < C; ++j)
    if (!sm.rescan_flag[j]) am_merge(win, sm.cgv[j], sm.cgi[j]);   // every thread: same merge order
  // (this rescan and argmax_allowed's are not shared: this one carries two accumulators)
  for (int j = 0; j < C; ++j) {
    if (!sm.rescan_flag[j]) continue;
    int clo, chi;
    chunk_range(r.V, j, clo, chi);
    // two accumulators updated by selects (a branch choosing one of two structs makes the
    // compiler address them through scratch)
    float wv = win.v, av = amb.v;
    int wx = win.i, ax = amb.i;
    sweep<T, VEC, 1>(r.ptr, clo, chi, [&](int i, float v) {
      const int gb = kmx - (int)floorf(v * r.sbin);
      if (gb <= gst) {
        const float sc = v * r.invT + gumbel(r.key, (uint32_t)i);
        const bool in = gb < gst;
        const bool bw = in && (sc > wv || (sc == wv && i < wx));
        const bool ba = !in && (sc > av || (sc == av && i < ax));
        wv = bw ? sc : wv;
        wx = bw ? i : wx;
        av = ba ? sc : av;
        ax = ba ? i : ax;
      }
    });
    win = ArgMax{wv, wx};
    amb = ArgMax{av, ax};
  }
  win = block_argmax(win, sm.sv, sm.si);
  amb = block_argmax(amb, sm.sv, sm.si);
  return (win.i != NO_TOKEN && (amb.v < win.v || (amb.v == win.v && amb.i > win.i))) ? win.i : -1;
}

// One pass over the row: m[k] = the mass (relative to the row max mx) of the tokens strictly above
// cv[k], for NC values at once, reduced over the workgroup.
template <typename T, bool VEC>
RT_DEVICE void mass_above(const RowConst<T>& r, float mx, const float (&cv)[NC], float (&m)[NC], Smem& sm) {
  float acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.f;
  sweep<T, VEC, ROW_UNR>(r.ptr, 0, r.V, [&](int, float v) {
    const float e = __expf((v - mx) * r.invT);
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] += v > cv[k] ? e : 0.f;
  });
#pragma unroll
  for (int k = 0; k < NC; ++k) m[k] = block_reduce<Sum>(acc[k], sm.red);
}

// Top-p slow path without a histogram (the rejected-j* case, ~1 - top_p of the rows):
// a token is inside the nucleus iff the mass of the tokens strictly more likely than it is below
// p * total (the reference's sorted-cumsum cut, restated), the same test the accept pass made for
// j*. Candidates = the chunks' best Gumbel tokens in score order; c1 = j* is out. ONE pass
// measures the mass above the next NC candidates; the first one inside, c*, is the answer unless
// a non-best token of a chunk ranked above c* (those chunks' bests are out) scores higher and is
// inside: those chunks are rescanned, their tokens' nucleus test decided from the known
// values (>= an inside candidate's value: in; <= an outside one's: out). Returns the token,
// or -1 when some token stays undecided or no candidate is inside (the histogram path decides).
template <typename T, bool VEC>
RT_DEVICE int nucleus_by_candidates(const RowConst<T>& r, float mx, float pz, float vj, Smem& sm) {
  if (threadIdx.x < C) {   // rank of chunk j's best by (score desc, index asc)
    const int j = threadIdx.x;
    int rank = 0;
    for (int q = 0; q < C; ++q)
      rank += (sm.cgv[q] > sm.cgv[j] || (sm.cgv[q] == sm.cgv[j] && sm.cgi[q] < sm.cgi[j])) ? 1 : 0;
    sm.ord[rank] = j;
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    const int gi = sm.cgi[sm.ord[1 + threadIdx.x]];
    sm.cv[threadIdx.x] = in_row(r, gi) ? rt::DT<T>::load(r.ptr + gi) : INFINITY;
  }
  if (threadIdx.x == 0) sm.flag = 0;
  __syncthreads();
  float cv[NC], m[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) cv[k] = sm.cv[k];
  mass_above<T, VEC>(r, mx, cv, m, sm);
  int kstar = -1;
  float v_in = INFINITY, v_out = vj;   // known: values >= v_in are inside, <= v_out outside
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const bool ok = cv[k] != INFINITY && m[k] < pz;
    if (ok) {
      if (kstar < 0) kstar = k;
      v_in = fminf(v_in, cv[k]);
    } else if (cv[k] != INFINITY) {
      v_out = fmaxf(v_out, cv[k]);
    }
  }
  if (kstar < 0) return -1;
  const int cs = sm.ord[1 + kstar];
  ArgMax best{sm.cgv[cs], sm.cgi[cs]};
  // chunks ranked above c* (their bests are outside): any token beating c* must be checked
  for (int q = 0; q <= kstar; ++q) {
    int lo, hi;
    chunk_range(r.V, sm.ord[q], lo, hi);
    sweep<T, VEC, 1>(r.ptr, lo, hi, [&](int i, float v) {
      const float sc = v * r.invT + gumbel(r.key, (uint32_t)i);
      if (sc > sm.cgv[cs] || (sc == sm.cgv[cs] && i < sm.cgi[cs])) {
        if (v >= v_in) {
          am_merge(best, sc, i);
        } else if (v > v_out) {             // undecided from the known values: test it exactly
          const int u = atomicAdd(&sm.flag, 1);
          if (u < NC) {
            sm.uv[u] = v;
            sm.us[u] = sc;
            sm.ui[u] = i;
          }
        }
      }
    });
  }
  best = block_argmax(best, sm.sv, sm.si);
  __syncthreads();
  const int nu = sm.flag;
  if (nu > NC) return -1;
  if (nu > 0) {   // one more pass: the mass above each undecided token
#pragma unroll
    for (int k = 0; k < NC; ++k) cv[k] = k < nu ? sm.uv[k] : INFINITY;
    mass_above<T, VEC>(r, mx, cv, m, sm);
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (k < nu && m[k] < pz) am_merge(best, sm.us[k], sm.ui[k]);
  }
  return best.i;
}

// Top-k from the chunk lists (no pass over the row): the union holds every chunk's top k, so its
// k-th largest key kg is the row's; every allowed token (key >= kg) is listed unless a chunk
// dropped ties AT kg (then -1). Plain top-k: the Gumbel argmax over the listed allowed tokens.
// With top-p inside the top-k set: the allowed tokens compacted in id order, the exact test —
// mass strictly above a token < p * allowed mass — and the Gumbel argmax over the nucleus (-1
// when more than NALLOW tokens are allowed). -1: the histogram path decides. Ends with a barrier
// (that path reuses the pool).
template <typename T>
RT_DEVICE int topk_from_lists(const RowConst<T>& r, float mx, Smem& sm) {
  const uint32_t* lk = sm.merged_keys();
  const int* li = sm.merged_ids();
  int cand = -1;
  const uint32_t kg = kth_key(lk, C * LCAP, r.k, r.KLO, sm.cnt3);
  if (threadIdx.x == 0) sm.fallback = 0;
  __syncthreads();
  if (threadIdx.x < C && (sm.tkn[threadIdx.x] >> 16) && (uint32_t)sm.tkk[threadIdx.x] == kg) sm.fallback = 1;
  __syncthreads();
  if (!sm.fallback && !(r.p < 1.f)) {
    ArgMax best{-INFINITY, NO_TOKEN};
    for (int e = threadIdx.x; e < C * LCAP; e += NT) {
      const uint32_t kk = lk[e];
      if (kk >= kg) am_merge(best, (okey_value(kk, r.KLO) - mx) * r.invT + gumbel(r.key, (uint32_t)li[e]), li[e]);
    }
    best = block_argmax(best, sm.sv, sm.si);
    cand = best.i != NO_TOKEN ? best.i : -1;
  } else if (!sm.fallback) {
    // lists are sorted by id, chunks in id order; each wave ranks 4 chunks with ballots
    uint32_t* ak = sm.allow_keys();
    int* ai = sm.allow_ids();
    float* aw = sm.allow_mass();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    constexpr int CPW = C / NWV, RPC = (LCAP + 63) / 64;
    int pos[CPW][RPC];
#pragma unroll
    for (int q = 0; q < CPW; ++q) {
      const int cc = wid * CPW + q;
      int run = 0;
#pragma unroll
      for (int s = 0; s < RPC; ++s) {
        const int j = lane + 64 * s;
        const bool al = j < LCAP && lk[cc * LCAP + j] >= kg;
        const unsigned long long m = __ballot(al);
        pos[q][s] = al ? run + __popcll(m & ((1ull << lane) - 1ull)) : -1;
        run += __popcll(m);
      }
      if (lane == 0) sm.ccnt[cc] = run;
    }
    __syncthreads();
    int tot = 0;
    for (int j = 0; j < C; ++j) tot += sm.ccnt[j];
    if (tot <= NALLOW) {
#pragma unroll
      for (int q = 0; q < CPW; ++q) {
        const int cc = wid * CPW + q;
        int base = 0;
        for (int j = 0; j < cc; ++j) base += sm.ccnt[j];
#pragma unroll
        for (int s = 0; s < RPC; ++s) {
          if (pos[q][s] >= 0) {
            const int e = cc * LCAP + lane + 64 * s;
            ak[base + pos[q][s]] = lk[e];
            ai[base + pos[q][s]] = li[e];
            aw[base + pos[q][s]] = __expf((okey_value(lk[e], r.KLO) - mx) * r.invT);
          }
        }
      }
      __syncthreads();
      const int t = threadIdx.x;
      const float my_w = t < tot ? aw[t] : 0.f;
      const float zsum = block_reduce<Sum>(my_w, sm.red);
      ArgMax best{-INFINITY, NO_TOKEN};
      if (t < tot) {
        const uint32_t mk = ak[t];
        float above = 0.f;
        for (int j = 0; j < tot; ++j) above += ak[j] > mk ? aw[j] : 0.f;
        if (above < r.p * zsum)
          am_merge(best, (okey_value(mk, r.KLO) - mx) * r.invT + gumbel(r.key, (uint32_t)ai[t]), ai[t]);
      }
      best = block_argmax(best, sm.sv, sm.si);
      cand = best.i != NO_TOKEN ? best.i : -1;
    }
  }
  __syncthreads();
  return cand;
}

// The slow path's threshold: the largest zthr such that {z >= zthr} holds the top k tokens and,
// of their mass, the top-p share. A 2048-bin histogram of z (count + mass) over the row's actual z
// range [zlo, 0] (not a fixed [-ZR, 0]: the values spread over all NB bins, so the LDS atomics of
// one workgroup rarely collide) -> the bin where the count or the mass crosses first -> a
// 2048-bin sub-histogram of that bin -> the crossing sub-bin's lower edge. Two passes over the
// row; -inf when nothing crosses (everything is allowed).
template <typename T, bool VEC>
RT_DEVICE float threshold_by_histogram(const RowConst<T>& r, float mx, float rmin, Smem& sm) {
  unsigned* hci = sm.counts_acc();
  unsigned long long* hmi = sm.mass_acc();
  const float* hm = sm.mass();
  const float zlo = fmaxf(-ZR, fminf((rmin - mx) * r.invT, -1e-3f));
  const float scale = NB / (-zlo * 1.0001f + 1e-6f);   // the row minimum lands inside the last bin
  sm.hist_clear<true>();
  sweep<T, VEC, ROW_UNR>(r.ptr, 0, r.V, [&](int, float v) {
    const float z = (v - mx) * r.invT;
    const float fb = -z * scale;
    if (fb < (float)NB) {
      const int bin = (int)fb;
      atomicAdd(&hci[bin], 1u);
      atomicAdd(&hmi[bin], mass_fixed(__expf(z)));
    }
  });
  sm.hist_to_float<true>();
  float tm = 0.f;
  for (int i = threadIdx.x; i < NB; i += NT) tm += hm[i];
  tm = block_reduce<Sum>(tm, sm.red);
  const float tk = r.use_k ? (float)r.k : NEVER;
  int bk = NB;
  float pre_c = 0.f, zk_mass = tm;
  if (r.use_k) {
    bk = crossing(sm, tk, NEVER);
    if (bk < NB) {
      zk_mass = sm.pb + hm[bk];
      pre_c = sm.pa;
    }
  }
  const float tp = r.p < 1.f ? r.p * zk_mass : NEVER;
  int bp = NB;
  float pre_m = 0.f;
  if (r.p < 1.f) {
    bp = crossing(sm, NEVER, tp);
    pre_m = sm.pb;
  }
  int bsel;
  bool by_count;
  float need;
  if (bk <= bp) {
    bsel = bk;
    by_count = true;
    need = tk - pre_c;
  } else {
    bsel = bp;
    by_count = false;
    need = tp - pre_m;
  }
  if (bsel >= NB) return -INFINITY;
  // sub-histogram of the selected bin
  __syncthreads();
  sm.hist_clear<true>();
  const float top_edge = -(float)bsel / scale, sub = scale * NB;
  sweep<T, VEC, ROW_UNR>(r.ptr, 0, r.V, [&](int, float v) {
    const float z = (v - mx) * r.invT;
    const float fb = -z * scale;
    if (fb >= (float)bsel && fb < (float)(bsel + 1)) {
      int sb = (int)((top_edge - z) * sub);
      sb = sb < 0 ? 0 : (sb >= NB ? NB - 1 : sb);
      atomicAdd(&hci[sb], 1u);
      atomicAdd(&hmi[sb], mass_fixed(__expf(z)));
    }
  });
  sm.hist_to_float<true>();
  const int cb = by_count ? crossing(sm, need, NEVER) : crossing(sm, NEVER, need);
  const int cc = cb < NB ? cb : NB - 1;
  return -(float)bsel / scale - (float)(cc + 1) / (scale * NB);
}

// Gumbel argmax over the allowed set {z >= zthr}. A chunk's best score over ALL its tokens
// (sm.cgv / cgi, from the chunk phase) is also its best allowed one whenever that token is
// allowed; only the chunks whose best is not (the rejected j*'s, ~1 - top_p of the others) are
// scanned again. Scores cgv = v/T + g differ from z + g by the row constant mx/T. An empty allowed
// set (rounding): the row argmax.
template <typename T, bool VEC>
RT_DEVICE int argmax_allowed(const RowConst<T>& r, const RowRec& d, float zthr, Smem& sm) {
  const float mx = d.ra.v;
  ArgMax best{-INFINITY, NO_TOKEN};
  if (threadIdx.x == 0) sm.nres = 0;
  __syncthreads();
  if (threadIdx.x < C) {
    const int j = threadIdx.x, gi = sm.cgi[j];
    const bool ok = in_row(r, gi) && (rt::DT<T>::load(r.ptr + gi) - mx) * r.invT >= zthr;
    if (!ok) sm.rescan_list[atomicAdd(&sm.nres, 1)] = j;
  }
  __syncthreads();
  for (int j = 0; j < C; ++j) {
    const int gi = sm.cgi[j];
    bool listed = false;
    for (int q = 0; q < sm.nres; ++q) listed |= sm.rescan_list[q] == j;
    if (!listed) am_merge(best, sm.cgv[j] - mx * r.invT, gi);     // every thread: same merge order
  }
  for (int q = 0; q < sm.nres; ++q) {
    int clo, chi;
    chunk_range(r.V, sm.rescan_list[q], clo, chi);
    sweep<T, VEC, 1>(r.ptr, clo, chi, [&](int i, float v) {
      const float z = (v - mx) * r.invT;
      if (z >= zthr) am_merge(best, z + gumbel(r.key, (uint32_t)i), i);
    });
  }
  best = block_argmax(best, sm.sv, sm.si);
  return best.i == NO_TOKEN ? d.ra.i : best.i;
}

// The decider's last words: the next launch's grid scale (top-p rows), the token (the path under
// RT_SMP_PROBE=5) and, with bookkeeping on, row b's decode_advance + next-step decode_prep from
// the step / position / length read with the parameters; the launch's last decider bumps `step`
// and re-arms the rows-done ticket.
template <typename T>
RT_DEVICE void finish_row(const SampleArgs& a, const RowConst<T>& r, const RowRec& d, int tok, int path, int64_t st,
                          int64_t pos_b, int ctx_b) {
  const int b = r.row;
  const rt::PrepArgs& pa = a.prep;
  if (r.hist && threadIdx.x == 0) {
    // next launch's grid: HB - 2 bins over the row's span (at most 8 / invT, where the mass
    // below is < e^-8 of the top token's), so a near-flat distribution (random-init weights)
    // still spreads over the bins instead of landing in one or two; never so fine that
    // floor(v * scale) leaves the int range
    const float mx = d.ra.v;
    const float span = fmaxf(fminf(mx - d.rmin, 8.f / r.invT), 1e-4f);
    const float sn = fminf((float)(HB - 2) / span, 1e6f / (fabsf(mx) + fabsf(d.rmin) + 1.f));
    publish(&r.w[W_SC], sn);
  }
  const int64_t pn = pos_b + 1;
  int64_t blk = 0;
  // the next K/V slot's block-table entry (thread 0) and the next step's embedding row (every
  // lane, 16 B) are requested together: one round trip for both
  if (a.adv && pa.slots != nullptr && threadIdx.x == 0) blk = rt::kv_block(pa, b, pn);
  if (a.adv && pa.res != nullptr)
    for (int j = threadIdx.x; j < pa.H / 8; j += NT) rt::embed_piece(pa, b, tok, j);
  if (threadIdx.x == 0) {
    a.tok[b] = a.probe == 5 ? path : tok;
    if (a.adv) {
      if (st < a.max_steps) a.out[st * a.B + b] = tok;
      a.ids[b] = tok;
      a.positions[b] = pn;
      a.ctx_lens[b] = ctx_b + 1;
      if (pa.slots != nullptr) {
        pa.slots[b] = rt::kv_slot(pa, blk, pn);
        pa.offsets[b] = pn + 1;
      }
    }
  }
  if (a.adv && threadIdx.x == 0) {   // the last decider of the launch advances the step counter
    int* done = reinterpret_cast<int*>(a.ws) + (size_t)a.B * W_ROW;
    const int prev = __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == a.B - 1) {
      publish(done, 0);
      *a.step = st + 1;
    }
  }
}

// 5 waves per SIMD (at most 102 VGPRs) asked for outright: every phase fits in that (no scratch),
// and it is what three of the four variants get anyway. Left to itself the scheduler drops the bf16
// vector variant to 4 waves and then spends whatever that allows (109 to 128 VGPRs, changing with
// any edit) on interleaving the whole-row passes.
template <typename T, bool VEC>
__global__ void __launch_bounds__(NT, 5) smp_kernel(SampleArgs a) {
  __shared__ Smem sm;
  using VT = typename RowVec<T>::type;
  const int b = blockIdx.x, c = blockIdx.y;
  int lo, hi;
  chunk_range(a.V, c, lo, hi);
  // this thread's first 16 B of the chunk, requested before the parameter loads (the chunk
  // pass cannot start until `temperature` arrives; its first round trip overlaps that one)
  constexpr bool PRELOAD = VEC && sizeof(T) == 2;
  VT pv{};
  if constexpr (PRELOAD) {
    if ((int)threadIdx.x < ((hi - lo) >> 3))
      pv = *reinterpret_cast<const VT*>(static_cast<const T*>(a.logits) + (size_t)b * a.ld + lo + 8 * threadIdx.x);
  }
  const VT* first = PRELOAD ? &pv : nullptr;
  const float temp = a.temperature[b];
  const int64_t off = a.offsets[b];
  const int64_t st = a.adv ? *a.step : 0;
  const float sgrid = fetch(&a.ws[(size_t)b * W_ROW + W_SC]);
  const int k = a.top_k[b];
  const float p = a.top_p[b];
  // the decider's step bookkeeping inputs come with the parameters (row b's decider is their
  // only writer, after every ticket of the row): no dependent trip at the end of the launch
  const int64_t pos_b = a.adv ? a.positions[b] : 0;
  const int ctx_b = a.adv ? a.ctx_lens[b] : 0;
  // the deciders rewrite offsets / step / the grid scale: every read of them completes before
  // this workgroup's ticket (take_ticket), and the deciders write only after every ticket of
  // their row / launch (one wait for all the parameter loads)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const RowConst<T> r = row_constants<T>(a, b, temp, off, sgrid, k, p);

  // ---- 1: every workgroup: its chunk's records, then the ticket ----
  const ChunkRec rec = chunk_records<T, VEC>(r, lo, hi, first, sm);
  if (r.hist) publish_chunk_hist<T, VEC>(r, c, lo, hi, first, rec.am.v, sm);
  if (r.lst) publish_chunk_topk<T>(r, c, lo, hi, sm);
  if (!take_ticket(r, c, rec, sm)) return;

  // ---- 2: the decider: the first path that settles the row ----
  float hv[HVQ];
  const RowRec d = load_row_records(r, sm, hv);
  const float mx = d.ra.v;
  int tok, path = PATH_PLAIN;
  if (!(r.temp > 0.f)) {
    tok = d.ra.i;
  } else if (!r.use_k && !(r.p < 1.f)) {
    tok = in_row(r, d.g.i) ? d.g.i : d.ra.i;     // no finite score: the row argmax
  } else {
    bool accepted = false;
    int cand = -1;
    if (!r.use_k && in_row(r, d.g.i)) {
      const Accept t = accept_test<T, VEC>(r, d, hv, sm);
      accepted = t.accepted;
      path = (accepted ? PATH_ACCEPT : PATH_RESCAN) + (t.decided ? 0 : PATH_EXACT_PASS);
      if (!accepted) {
        cand = nucleus_from_chunk_hists<T, VEC>(r, t.pz, sm);
        if (cand < 0) {
          cand = nucleus_by_candidates<T, VEC>(r, mx, t.pz, t.vj, sm);
          path += PATH_CANDIDATES - PATH_RESCAN;
        }
      }
    }
    if (r.lst) cand = topk_from_lists(r, mx, sm);
    if (accepted) {
      tok = d.g.i;
    } else if (cand >= 0) {
      tok = cand;
    } else {
      path = (path / PATH_EXACT_PASS) * PATH_EXACT_PASS + PATH_HISTOGRAM;
      tok = argmax_allowed<T, VEC>(r, d, threshold_by_histogram<T, VEC>(r, mx, d.rmin, sm), sm);
    }
  }

  // ---- 3: the token and this row's step bookkeeping ----
  finish_row(a, r, d, tok, path, st, pos_b, ctx_b);
}

// one launch of the (B, C) grid on filled arguments
int launch(SampleArgs a, bool is_bf16, hipStream_t stream) {
  if (a.B == 0) return 0;
  if (a.V < 1) return -1;
  const size_t esz = is_bf16 ? 2 : 4;
  const bool vec = ((uintptr_t)a.logits % 16 == 0) && ((a.ld * esz) % 16 == 0);
  static const int probe = getenv("RT_SMP_PROBE") ? atoi(getenv("RT_SMP_PROBE")) : 0;
  a.probe = probe;
  const dim3 g(a.B, C);
  if (is_bf16) {
    if (vec) hipLaunchKernelGGL((smp_kernel<uint16_t, true>), g, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL((smp_kernel<uint16_t, false>), g, dim3(NT), 0, stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((smp_kernel<float, true>), g, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL((smp_kernel<float, false>), g, dim3(NT), 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

SampleArgs sample_args(int64_t* tok, const void* logits, int B, int V, int64_t ld_row, const float* temperature,
                       const float* top_p, const int* top_k, const int64_t* seeds, const int64_t* offsets, float* ws) {
  return SampleArgs{tok, ws, logits, V, ld_row, temperature, top_p, top_k, seeds, offsets, B};   // the rest: zero
}
}  // namespace

int sample_workspace_floats(int B) { return B * W_ROW + 4; }

int launch_sample(int64_t* out, const void* logits, bool is_bf16, int B, int V, int64_t ld_row,
                  const float* temperature, const float* top_p, const int* top_k, const int64_t* seeds,
                  const int64_t* offsets, float* ws, hipStream_t stream) {
  return launch(sample_args(out, logits, B, V, ld_row, temperature, top_p, top_k, seeds, offsets, ws), is_bf16, stream);
}

// The captured decode step's sampler + bookkeeping (decode_advance + decode_prep semantics).
int launch_sample_advance(int64_t* tok, const void* logits, bool is_bf16, int B, int V, int64_t ld_row,
                          const float* temperature, const float* top_p, const int* top_k, const int64_t* seeds,
                          int64_t* offsets, float* ws, int64_t* out, int64_t* ids, int64_t* positions, int* ctx_lens,
                          int64_t* step, int max_steps, int64_t* slots, void* res, const int* block_tables,
                          const void* embed, int max_blocks, int BS, int H, int64_t vocab, hipStream_t stream) {
  SampleArgs a = sample_args(tok, logits, B, V, ld_row, temperature, top_p, top_k, seeds, offsets, ws);
  a.adv = 1;
  a.out = out;
  a.ids = ids;
  a.positions = positions;
  a.ctx_lens = ctx_lens;
  a.step = step;
  a.max_steps = max_steps;
  if (res != nullptr) {   // the next step's prep: its offsets are the sampler's, rewritten by the deciders
    a.prep = rt::PrepArgs{slots, offsets, (uint16_t*)res, block_tables, (const uint16_t*)embed, max_blocks, BS, H,
                          vocab};
    if (!rt::prep_args_ok(a.prep)) return -3;
  }
  return launch(a, is_bf16, stream);
}
