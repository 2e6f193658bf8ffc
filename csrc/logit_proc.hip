// Logit processors: logit_bias, repetition penalty, frequency / presence penalties, applied in
// place to the logits of one sampling step, BEFORE K6 (csrc/sampling.hip) samples from them.
//
// Inside the captured decode step the tokens generated so far live only on the device (K6 writes
// out[step, b] and advances step; the host sees them every sync_every / 2 replays), so the
// penalties are computed here, in the graph, from that device-resident history:
//
//   S(b) = hist[b, :hist_len[b]] ++ out[0:*step, b]          (time order; step == nullptr: host part only)
//   repetition set = the last min(last_n, 2048) tokens of S  (last_n < 0: 2048; 0: none)
//   counted reply  = the last 2048 tokens of S[reply_from[b]:]
//
// per named token, in fp32 on the stored logit l (-inf stays -inf), rounded once on the store:
//   l += bias;  in the repetition set: l = l > 0 ? l / rp : l * rp;  count c > 0: l -= fp * c, l -= pp
//
// One workgroup per row, never a pass over V: at most 2048 history tokens (the reply is a suffix
// of S, so both windows lie inside the last 2048 tokens) and 300 bias entries go into a 4096-slot
// open-addressing table in LDS (key = token id, home slot = id & 4095, linear probing; <= 2348
// keys, so a probe always ends). Counts and flags are INTEGER LDS atomics, as K6's histograms:
// they do not depend on arrival order, and each occupied slot then has exactly one writer of
// logits[b, tok] — deterministic. Elements no token names are never read or written; a row whose
// parameters are all neutral returns at once. No cross-workgroup hand-off, plain vector stores.
#include "common.h"

namespace {
using namespace rt;

constexpr int LP_WINDOW = 2048;     // ops.LOGIT_PROC_WINDOW
constexpr int LP_MAX_BIAS = 300;    // ops.LOGIT_PROC_MAX_BIAS
constexpr int LP_SLOTS = 4096;
// 1024 threads per row: the kernel is a chain of dependent trips (id -> LDS CAS -> atomics; slot ->
// logit -> store), so its time is trips per thread: 2 tokens and 4 slots here. 256 threads took
// 13.8 µs for a 2048-token window against 6.6 µs (profiles/r08/logit_processors/README.md).
constexpr int LP_NT = 1024;
// slot value: bits 0..15 reply count (<= 2048), bit 16 "in the repetition set", bits 17.. bias entry + 1
constexpr unsigned LP_REP = 1u << 16;
constexpr int LP_BIAS_SHIFT = 17;

struct LogitProcArgs {
  void* logits;
  int64_t ld;
  int V;
  const int* hist;
  int hist_cap;
  const int* hist_len;
  const int* reply_from;
  const float* rp;
  const int* last_n;
  const float* pp;
  const float* fp;
  const int* bias_tok;
  const float* bias_val;
  const int* bias_n;
  int bias_cap;
  const int64_t* out;     // [max_steps, out_ld] device-side token record, or nullptr
  const int64_t* step;    // device step counter, or nullptr (host history only)
  int max_steps;
  int out_ld;
};

// slot of `tok` (inserted if new). The table never fills (<= 2348 of 4096); the bound only keeps
// a broken caller from spinning.
RT_DEVICE int lp_slot(int* keys, int tok) {
  int s = tok & (LP_SLOTS - 1);
  for (int p = 0; p < LP_SLOTS; ++p) {
    const int prev = atomicCAS(&keys[s], -1, tok);
    if (prev == -1 || prev == tok) return s;
    s = (s + 1) & (LP_SLOTS - 1);
  }
  return -1;
}

template <typename T>
__global__ void __launch_bounds__(LP_NT) logit_proc_kernel(LogitProcArgs a) {
  __shared__ int keys[LP_SLOTS];
  __shared__ unsigned vals[LP_SLOTS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float rp = a.rp[b], pp = a.pp[b], fp = a.fp[b];
  const int nb = min(min(max(a.bias_n[b], 0), a.bias_cap), LP_MAX_BIAS);
  const int ln = a.last_n[b];
  const int n_rep_want = (rp == 1.f || ln == 0) ? 0 : (ln < 0 ? LP_WINDOW : min(ln, LP_WINDOW));
  const bool counted = pp != 0.f || fp != 0.f;
  if (n_rep_want == 0 && !counted && nb == 0) return;     // neutral row (uniform: no barrier passed)

  for (int s = tid; s < LP_SLOTS; s += LP_NT) {
    keys[s] = -1;
    vals[s] = 0u;
  }
  __syncthreads();

  // phase 1: bias entries. Only this phase writes the bias field, so atomicMax keeps the LAST
  // entry of a token named twice (a dict has none; the oracle does the same).
  const int* btok = a.bias_tok + (size_t)b * a.bias_cap;
  for (int j = tid; j < nb; j += LP_NT) {
    const int tok = btok[j];
    if (tok < 0 || tok >= a.V) continue;
    const int s = lp_slot(keys, tok);
    if (s >= 0) atomicMax(&vals[s], (unsigned)(j + 1) << LP_BIAS_SHIFT);
  }
  __syncthreads();

  // phase 2: history. Index i of S: host part first, then the graph's own record.
  const int n_host = min(max(a.hist_len[b], 0), a.hist_cap);
  int n_dev = 0;
  if (a.step != nullptr && a.out != nullptr) n_dev = (int)min<int64_t>(max<int64_t>(*a.step, 0), a.max_steps);
  const int total = n_host + n_dev;
  const int rep_lo = total - min(n_rep_want, total);
  const int rf = min(max(a.reply_from[b], 0), n_host);
  const int cnt_lo = counted ? total - min(total - rf, LP_WINDOW) : total;
  const int* hist = a.hist + (size_t)b * a.hist_cap;
  for (int i = min(rep_lo, cnt_lo) + tid; i < total; i += LP_NT) {
    const int64_t t64 = i < n_host ? (int64_t)hist[i] : a.out[(size_t)(i - n_host) * a.out_ld + b];
    if (t64 < 0 || t64 >= a.V) continue;
    const int s = lp_slot(keys, (int)t64);
    if (s < 0) continue;
    if (i >= rep_lo) atomicOr(&vals[s], LP_REP);
    if (i >= cnt_lo) atomicAdd(&vals[s], 1u);
  }
  __syncthreads();

  // phase 3: one thread per occupied slot rewrites its logit.
  T* row = reinterpret_cast<T*>(a.logits) + (size_t)b * a.ld;
  const float* bval = a.bias_val + (size_t)b * a.bias_cap;
  for (int s = tid; s < LP_SLOTS; s += LP_NT) {
    const int tok = keys[s];
    if (tok < 0) continue;
    const unsigned v = vals[s];
    float l = DT<T>::load(row + tok);
    if (l == -INFINITY) continue;
    const int bi = (int)(v >> LP_BIAS_SHIFT);
    if (bi > 0) l += bval[bi - 1];
    if (v & LP_REP) l = l > 0.f ? l / rp : l * rp;
    const int c = (int)(v & 0xffffu);
    if (c > 0) {
      l -= __fmul_rn(fp, (float)c);     // no fma: the fp32 reference rounds the product
      l -= pp;
    }
    DT<T>::store(row + tok, l);
  }
}
}  // namespace

// dtype: 0 = bf16, 1 = fp32 logits. hist [B, hist_cap] int32; bias_tok / bias_val [B, bias_cap].
int launch_logit_proc(void* logits, int dtype, int B, int V, int64_t ld, const int* hist, int hist_cap,
                      const int* hist_len, const int* reply_from, const float* rp, const int* last_n, const float* pp,
                      const float* fp, const int* bias_tok, const float* bias_val, const int* bias_n, int bias_cap,
                      const int64_t* out, const int64_t* step, int max_steps, int out_ld, hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0 || ld < V || hist_cap < 0 || bias_cap < 0 || (dtype != 0 && dtype != 1)) return -1;
  if ((out == nullptr) != (step == nullptr)) return -2;
  if (out != nullptr && (max_steps < 0 || out_ld < B)) return -3;
  LogitProcArgs a{logits, ld,       V,        hist,   hist_cap, hist_len, reply_from, rp,        last_n, pp,
                  fp,     bias_tok, bias_val, bias_n, bias_cap, out,      step,       max_steps, out_ld};
  if (dtype == 0)
    hipLaunchKernelGGL(logit_proc_kernel<uint16_t>, dim3(B), dim3(LP_NT), 0, stream, a);
  else
    hipLaunchKernelGGL(logit_proc_kernel<float>, dim3(B), dim3(LP_NT), 0, stream, a);
  return 0;
}
