// Logprobs of one sampling step: the chosen token's log-probability and the n_top most likely
// tokens with theirs, on the logits AS K6 (csrc/sampling.hip) SAMPLED FROM THEM: after the logit
// processors, before temperature / top-k / top-p. l[i] = the stored bf16 / fp32 logit as fp32:
//
//   lse    = m + log(sum_i exp(l[i] - m)),  m = max_i l[i]        (a -inf logit adds 0)
//   tok_lp = l[tok] - lse                                         (tok outside [0, V): NaN, nothing read)
//   top    = the n_top largest l, value descending then token id ascending (K6's argmax tie rule,
//            am_merge), each with l - lse; entries past min(n_top, V): id -1, lp -inf
//
// Inside the captured decode step the logits live one replay, so this runs in the graph, after K6:
// K6 does not write the logits and neither do these kernels. Two launches, the kernel boundary the
// only hand-off (no ticket, no last arriver: only batches that ask for logprobs pay for it):
//
//   logprob_chunks (B, NCH): chunk max, sum exp(l - chunk max) and the chunk's top
//       min(n_top, chunk length) (key, id) pairs in id order;
//   logprob_merge  (B):      lse from the NCH (max, sum) pairs IN CHUNK ORDER, the row's top n_top
//       of the <= NCH x 20 candidates, the chosen token's logit, the record row.
//
// Every reduction has a fixed order and the selections are exact on order keys (okey), so the
// result does not depend on which workgroup ran first. Rows with n_top < 0 return before any
// barrier and write nothing. Global memory is written with plain vector stores only.
#include "logprobs_plan.h"
#include "sampling_prims.h"

namespace {
using namespace rt;
using namespace smp;
using namespace lpr;

constexpr int EPT = CHUNK / NT;                          // 8 consecutive elements per thread
constexpr int MSLOTS = MAX_CHUNKS * MAX_TOP;             // candidate slots of a row
constexpr int SPT = (MSLOTS + NT - 1) / NT;              // 3 consecutive slots per thread
static_assert(EPT == 8 && CHUNK == EPT * NT, "a thread owns one 16-byte bf16 vector / two fp32 vectors");

struct LogprobArgs {
  const void* logits;
  int64_t ld;
  int V, nch;
  const int* n_top;
  float* ws;
  // merge
  const int64_t* ids;      // eager form: [B] chosen tokens, record row 0
  const int64_t* out;      // graph form: [max_steps, out_ld] and the device step counter (K6 has
  const int64_t* step;     // advanced it: the token is out[*step - 1, b], the record row *step - 1)
  int max_steps, out_ld;
  float* tok_lp;           // [steps, rec_ld]
  int* top_id;             // [steps, rec_ld, rec_cols]
  float* top_lp;
  int rec_ld, rec_cols;
};

// Exclusive prefix over the workgroup's threads of a packed pair of counts (hi << 16 | lo, each
// total <= 4096), in thread order; *total = the sum. scr: NWV ints.
RT_DEVICE int scan_excl(int v, int* scr, int* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int x = __shfl_up(s, o, 64);
    if (lane >= o) s += x;
  }
  __syncthreads();
  if (lane == 63) scr[wid] = s;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NWV; ++w) {
    const int x = scr[w];
    before += w < wid ? x : 0;
    all += x;
  }
  *total = all;
  return before + s - v;
}

// The thread's EPT consecutive elements of the chunk [0, n) at `p` as fp32 (absent: -inf):
// 16-byte loads where the vector is whole and aligned, element-wise otherwise (the tail).
template <typename T>
RT_DEVICE void load_elems(const T* p, int e0, int n, bool aligned, float* v) {
  constexpr int EPV = 16 / (int)sizeof(T);
#pragma unroll
  for (int q = 0; q < EPT / EPV; ++q) {
    const int i0 = e0 + q * EPV;
    if (aligned && i0 + EPV <= n) {
      if constexpr (sizeof(T) == 2) {
        const short8 x = *reinterpret_cast<const short8*>(p + i0);
#pragma unroll
        for (int j = 0; j < EPV; ++j) v[q * EPV + j] = bf2f((uint16_t)x[j]);
      } else {
        const float4_ x = *reinterpret_cast<const float4_*>(p + i0);
#pragma unroll
        for (int j = 0; j < EPV; ++j) v[q * EPV + j] = x[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < EPV; ++j) v[q * EPV + j] = i0 + j < n ? DT<T>::load(p + i0 + j) : -INFINITY;
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(NT) logprob_chunks_kernel(LogprobArgs a) {
  constexpr int KLO = sizeof(T) == 2 ? 16 : 0;
  __shared__ uint32_t keys[CHUNK];
  __shared__ float red[NWV];
  __shared__ int cnt3[2 * 3 * NWV], scn[NWV];
  const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int nt = min(a.n_top[b], MAX_TOP);
  if (nt < 0) return;     // row without logprobs (uniform: no barrier passed)
  const int lo = c * CHUNK, n = min(a.V - lo, CHUNK);
  if (c >= a.nch || n <= 0) return;
  const T* p = static_cast<const T*>(a.logits) + (size_t)b * a.ld + lo;
  const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  const int e0 = tid * EPT;

  float v[EPT];
  uint32_t kk[EPT];
  load_elems<T>(p, e0, n, aligned, v);
  float tm = -INFINITY;
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const bool in = e0 + j < n;
    // + 0.f: -0.0 takes +0.0's key (they tie in value). 0: below every value's key
    kk[j] = in ? okey(v[j] + 0.f, KLO) : 0u;
    keys[e0 + j] = kk[j];
    tm = fmaxf(tm, v[j]);
  }
  const float m = block_reduce<Max>(tm, red);
  float ts = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int j = 0; j < EPT; ++j) ts += expf(v[j] - m);     // absent and banned: exp(-inf) = 0
  }
  const float s = block_reduce<Sum>(ts, red);

  float* w = a.ws + (size_t)b * WS_ROW + (size_t)c * WS_REC;
  const int need = min(nt, n);
  if (need > 0) {     // (uniform)
    // the chunk's need-th largest key; everything above it is listed, its ties by lower id
    const uint32_t kc = kth_key(keys, n, need, KLO, cnt3);
    int na = 0, ne = 0;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      na += kk[j] > kc;
      ne += kk[j] == kc && e0 + j < n;
    }
    int total;
    const int pre = scan_excl((na << 16) | ne, scn, &total);
    const int ties = need - (total >> 16);     // ties listed: the first `ties` in id order
    int pa = pre >> 16, pe = pre & 0xffff;
    uint32_t* wk = reinterpret_cast<uint32_t*>(w) + WS_KEY;
    int* wi = reinterpret_cast<int*>(w) + WS_ID;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      const bool above = kk[j] > kc, tie = kk[j] == kc && e0 + j < n;
      const int slot = pa + min(pe, ties);     // listed elements before this one: id order
      if ((above || (tie && pe < ties)) && slot < MAX_TOP) {
        wk[slot] = kk[j];
        wi[slot] = lo + e0 + j;
      }
      pa += above;
      pe += tie;
    }
  }
  if (tid == 0) {
    w[WS_M] = m;
    w[WS_S] = s;
    reinterpret_cast<int*>(w)[WS_N] = need;
  }
}

template <typename T>
__global__ void __launch_bounds__(NT) logprob_merge_kernel(LogprobArgs a) {
  constexpr int KLO = sizeof(T) == 2 ? 16 : 0;
  __shared__ uint32_t lk[SPT * NT];
  __shared__ uint32_t sel_k[MAX_TOP];
  __shared__ int sel_i[MAX_TOP];
  __shared__ int cnt3[2 * 3 * NWV], scn[NWV];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nt = min(a.n_top[b], MAX_TOP);
  if (nt < 0) return;     // (uniform: no barrier passed)
  int64_t tok;
  int64_t rec = 0;
  if (a.step != nullptr) {
    rec = *a.step - 1;     // K6 recorded out[rec] and advanced the counter
    if (rec < 0 || rec >= a.max_steps) return;
    tok = a.out[(size_t)rec * a.out_ld + b];
  } else {
    tok = a.ids[b];
  }
  const float* wrow = a.ws + (size_t)b * WS_ROW;

  // lse, the chunks in chunk order (every thread the same arithmetic on the same words)
  float M = -INFINITY;
  for (int c = 0; c < a.nch; ++c) M = fmaxf(M, wrow[(size_t)c * WS_REC + WS_M]);
  float S = 0.f;
  for (int c = 0; c < a.nch; ++c) {
    const float mc = wrow[(size_t)c * WS_REC + WS_M];
    if (mc > -INFINITY) S += wrow[(size_t)c * WS_REC + WS_S] * expf(mc - M);
  }
  const float lse = M + logf(S);

  // candidates: slot q = chunk * 20 + j, ids ascending in slot order (chunks are id ranges and
  // every chunk listed in id order); slots past a chunk's count hold key 0
  const int nslots = a.nch * MAX_TOP;
  uint32_t kk[SPT];
  int ii[SPT];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int q = tid * SPT + j;
    kk[j] = 0u;
    ii[j] = -1;
    if (q < nslots) {
      const int c = q / MAX_TOP, r = q - c * MAX_TOP;
      const float* w = wrow + (size_t)c * WS_REC;
      const int cn = min(max(reinterpret_cast<const int*>(w)[WS_N], 0), MAX_TOP);
      if (r < cn) {
        kk[j] = reinterpret_cast<const uint32_t*>(w)[WS_KEY + r];
        ii[j] = reinterpret_cast<const int*>(w)[WS_ID + r];
      }
    }
    lk[q] = kk[j];
  }
  __syncthreads();
  const int need = min(nt, a.V);
  if (need > 0) {     // (uniform)
    const uint32_t kg = kth_key(lk, nslots, need, KLO, cnt3);
    int na = 0, ne = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      na += kk[j] > kg;
      ne += kk[j] == kg && ii[j] >= 0;
    }
    int total;
    const int pre = scan_excl((na << 16) | ne, scn, &total);
    const int ties = need - (total >> 16);
    int pa = pre >> 16, pe = pre & 0xffff;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const bool above = kk[j] > kg, tie = kk[j] == kg && ii[j] >= 0;
      const int slot = pa + min(pe, ties);
      if ((above || (tie && pe < ties)) && slot < MAX_TOP) {
        sel_k[slot] = kk[j];
        sel_i[slot] = ii[j];
      }
      pa += above;
      pe += tie;
    }
  }
  __syncthreads();

  const size_t r0 = (size_t)rec * a.rec_ld + b;
  if (tid < MAX_TOP) {
    int id = -1, rank = tid;
    float lp = -INFINITY;
    if (tid < need) {     // sel is in id order: rank by (key descending, position ascending)
      const uint32_t k = sel_k[tid];
      rank = 0;
      for (int j = 0; j < need; ++j) rank += sel_k[j] > k || (sel_k[j] == k && j < tid);
      id = sel_i[tid];
      lp = okey_value(k, KLO) - lse;
    }
    a.top_id[r0 * a.rec_cols + rank] = id;
    a.top_lp[r0 * a.rec_cols + rank] = lp;
  }
  if (tid == 64) {
    float l = __builtin_nanf("");
    if (tok >= 0 && tok < a.V) l = DT<T>::load(static_cast<const T*>(a.logits) + (size_t)b * a.ld + tok) - lse;
    a.tok_lp[r0] = l;
  }
}
}  // namespace

// dtype: 0 = bf16, 1 = fp32 logits [B, V] (row stride ld). n_top [B] (< 0: row off). ws:
// lpr::workspace_words(B) floats. Records tok_lp [rec_steps, rec_ld], top_id / top_lp
// [rec_steps, rec_ld, rec_cols]. Eager form: ids [B], record row 0; graph form: out
// [max_steps, out_ld] + device step, record row *step - 1. Negative: refused (logprobs_plan.h).
int launch_token_logprobs(const void* logits, int dtype, int B, int V, int64_t ld, const int* n_top, float* ws,
                          int64_t ws_words, const int64_t* ids, const int64_t* out, const int64_t* step,
                          int max_steps, int out_ld, float* tok_lp, int* top_id, float* top_lp, int rec_steps,
                          int rec_ld, int rec_cols, hipStream_t stream) {
  if (B <= 0) return 0;
  const lpr::LogprobPlan pl = lpr::plan_logprobs(B, V, ld, dtype, rec_cols, rec_ld, rec_steps, ids != nullptr,
                                                 out != nullptr, step != nullptr, max_steps, out_ld, ws_words);
  if (pl.rc != 0) return pl.rc;
  LogprobArgs a{logits, ld,        V,      pl.nch, n_top,  ws,     out != nullptr ? nullptr : ids, out, step,
                max_steps, out_ld, tok_lp, top_id, top_lp, rec_ld, rec_cols};
  if (dtype == 0) {
    hipLaunchKernelGGL(logprob_chunks_kernel<uint16_t>, dim3(B, pl.nch), dim3(NT), 0, stream, a);
    hipLaunchKernelGGL(logprob_merge_kernel<uint16_t>, dim3(B), dim3(NT), 0, stream, a);
  } else {
    hipLaunchKernelGGL(logprob_chunks_kernel<float>, dim3(B, pl.nch), dim3(NT), 0, stream, a);
    hipLaunchKernelGGL(logprob_merge_kernel<float>, dim3(B), dim3(NT), 0, stream, a);
  }
  return 0;
}
