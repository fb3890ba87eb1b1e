// Training attention for the learn step: causal + key-padding mask, softmax in fp32, post-softmax
// dropout (x-transformers Attend, called from WorldModelActorCritic.forward in Agent.learn,
// x_transformers_rl.py:928-935 with mask = arange(n) < episode_lens, :908-909).
//
// All products run on the f32 matrix cores (v_mfma_f32_16x16x4_f32):
//   forward   S = Q K^T, online softmax, O = P~ V              (flash style, no n x n in HBM)
//   backward  D = rowsum(dO * O); dK, dV per key tile; dQ per query tile (no atomics, deterministic)
// Geometry: 64-row tiles, 4 waves x 16 rows; K/V (or Q/dO) tiles staged in LDS with a 2-float
// row pad; the probability tile crosses LDS once per wave to turn the MFMA C layout (rows on
// lane groups) into the A layout (rows on lanes), in a 66-float-stride image (conflict-free read).
// Dropout keep bits, with c2 = offset + b*H + h (sub = the decoder layer / fractal level):
//   byte mode (256 p an integer, e.g. p = 0.25): byte (i & 3) of word ((j >> 4) & 3) of
//     philox(seed; i >> 2, 16 (j >> 6) + (j & 15), c2, FIELD_DROPOUT << 24 | (sub | 1 << 23)) >= 256 p —
//     one block covers rows 4 (i >> 2) + 0..3 and columns j, j + 16, j + 32, j + 48 of a 64-key tile:
//     exactly the 16 scores one lane holds in the forward and dQ kernels (one block per lane and tile)
//   word mode: word (i & 3) of philox(seed; i >> 2, j, c2, FIELD_DROPOUT << 24 | sub) >= p 2^32.
// Attention sinks (AttnProblem.mem_kv M learned memory key / value rows per kv head, zero_kv Z one all-zero
// key / value): columns every row sees, folded into the online softmax before the key-tile loop — Z is the
// initial state m = 0, l = 1, o = 0 and the memory rows are one 16-column sub-tile — so lse includes them
// and the backward kernels of the real keys (which recompute P from lse and use D = rowsum(dO * O)) stay
// as they are.  k_attn_sink_bwd adds the sink term of dQ and forms dmem_k / dmem_v.
//   keep bit of memory column m at row i, in either mode: word (i & 3) of
//     philox(seed; i >> 2, 0x80000000 | m, c2, c3) >= p 2^32, c3 the call's own (byte mode: its flag set).
//   A real key's c1 is j or 16 (j >> 6) + (j & 15) with j < n < 2^31: no real key draws from a counter
//   with bit 31 of c1 set, and the real keys' bits do not depend on M.  The zero key's value is 0: no bit.
// ALiBi (AttnProblem.alibi, slopes [H]): the score of row i and real key j becomes scale q_i . k_j -
// slope[h] (i - j), i and j the positions inside the episode (the lane holds both in every score loop), added
// before the mask select; the sinks take no bias and the keep bits do not change.  The backward kernels
// recompute P with the same term; dS, D and the scale factors of dQ / dK are as without it (the bias has no
// gradient).  Compile-time forms of the forward, k_attn_bwd_dkdv and k_attn_bwd_dq on top of the GQA ones
// (which serve Hkv = H too); k_attn_bwd_fused has none.  A dead row's filled scores are all the same -max
// whatever the bias was: k_attn_dead_fwd / k_attn_dead_bwd are unchanged.
// Logit soft-clamp (AttnProblem.softclamp = c > 0, x-transformers attn_softclamp_logits): with x the score
// above (bias included), s = c tanh(x / c) for the real keys and the memory columns, before the mask
// select; the zero key's 0 stays 0 and the keep bits do not change.  lse is that of the clamped scores.  The
// backward kernels recompute t = tanh(x / c) in the expression that forms s, so P is that of the forward,
// and hand on dX = dS (1 - t^2) where they handed on dS: dQ, dK and dmem_k take it with their scale factors,
// dV and dmem_v do not change.  Compile-time CAP forms on top of the ALiBi ones (the slope is 0 when there
// are no slopes), and of k_attn_sink_bwd; k_attn_bwd_fused has none.  tanhf, not 1 - 2 / (1 + e^2y): at c = 50
// the arguments are near 0.02 and the absolute error of t is multiplied by c.  A dead row's filled scores
// are the same -max whatever the clamp did: k_attn_dead_fwd / k_attn_dead_bwd are unchanged.
#include <cmath>

#include "kernels.h"
#include "philox.h"

namespace xtrl {
namespace {

constexpr int TQ = 64, TK = 64, PST = 66;

typedef float f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4v mfma16(float a, float b, f32x4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ uint32_t keep_word(uint64_t seed, uint32_t off, uint32_t c3, int i, int j) {
  const u32x4_t r = philox4x32_10((uint32_t)(i >> 2), (uint32_t)j, off, c3, seed);
  const int w = i & 3;
  return w == 0 ? r.x : (w == 1 ? r.y : (w == 2 ? r.z : r.w));
}
__device__ __forceinline__ uint32_t qword(const u32x4_t& u, int r) {
  return r == 0 ? u.x : (r == 1 ? u.y : (r == 2 ? u.z : u.w));
}
// byte-mode keep byte (row & 3) of word (16-column group) of a lane's block
__device__ __forceinline__ uint32_t qbyte(const u32x4_t& u, int word, int r) {
  return (qword(u, word) >> (8 * r)) & 0xFFu;
}

struct AttnArgs {
  const float *Q, *K, *V, *O, *LSE, *dO, *Dl, *G;
  float *Oout, *LSEout, *dQ, *dK, *dV, *Dout, *OGout;
  float* dQp;         // k_attn_bwd_dkdv<DH, true>: per-key-tile dQ partials [n_key_tiles][b H][n][DH]
  const int32_t* ep_off;   // packed rows: episode b's tokens are rows ep_off[b] .. + min(lens[b], n) - 1
  const int32_t* lens;
  int H, n;
  AttnLayout in, out, grad, gate;   // q/k/v; o/do/og; dq/dk/dv; gate
  float scale, inv_keep;
  uint32_t thresh;    // keep iff word >= thresh (thresh = 0: no dropout)
  uint32_t thresh8;   // != 0: byte mode, keep iff byte >= thresh8
  uint64_t seed;
  uint32_t offset;
  uint32_t c3;        // rng_c3(FIELD_DROPOUT, layer); byte mode: rng_c3(FIELD_DROPOUT, layer | 1 << 23)
  int causal;
  int window;         // sliding window W: key j visible to query i only if i - j <= W (NO_WINDOW: none)
  // grouped-query attention (read by the GQA = true instantiations only): K, V in layout kv and dK, dV
  // in layout kvgrad hold Hkv heads; query head h reads kv head kv_head_of(h, Hkv)
  int Hkv;
  AttnLayout kv, kvgrad;
  // attention sinks (read by the SINK = true forward and by k_attn_sink_bwd / k_attn_sink_reduce only)
  const float *MK, *MV;   // [Hkv][M][dh]
  float *dMKp, *dMVp;     // per-(b, h) partials [b H][M][dh]
  float *dMK, *dMV;       // [Hkv][M][dh]
  int M, Z, dm_accum;
  // ALiBi (read by the ALIBI = true instantiations only): slope per query head [H]; the score of row i and real
  // key j (positions inside the episode) is scale q_i . k_j - alibi[h] (i - j); the sinks take no bias
  const float* alibi;
  // logit soft-clamp (read by the CAP = true instantiations only): c and 1 / c
  float cap, inv_cap;
};
constexpr uint32_t SINK_C1 = 0x80000000u;   // c1 of a memory column's keep word: SINK_C1 | m
constexpr int NO_WINDOW = 1 << 30;   // (i - j <= NO_WINDOW always holds; band tile ranges become the causal ones)

// first row of episode b in layout L: b * sb (padded [b][n] tokens), or ep_off[b] rows (packed)
__device__ __forceinline__ int64_t ebase(const AttnArgs& a, const AttnLayout& L, int b) {
  return a.ep_off ? (int64_t)a.ep_off[b] * L.si : (int64_t)b * L.sb;
}

// ---------------------------------------------------------------------------------------------
// GQA = true (Hkv < H): the K / V base is the kv head's, in its own layout; nothing else changes
// SINK = true (M + Z > 0): the sinks enter the softmax state before the key-tile loop (instantiations of
// their own: the forms without sinks keep their code)
// ALIBI = true (a.alibi set, always with GQA: the kv head mapping at run time, Hkv = H included): the
// head's distance penalty joins each real key's score before the mask select
// CAP = true (a.cap > 0, always with ALIBI, whose slope is 0 when a.alibi is NULL): the real keys' and the
// memory columns' scores become cap tanh(score / cap) before the mask select
template <int DH, bool GQA = false, bool SINK = false, bool ALIBI = false, bool CAP = false>
__global__ __launch_bounds__(256) void k_attn_fwd(const AttnArgs a) {
  static_assert(GQA || !ALIBI, "the ALiBi forms take the kv head mapping at run time");
  static_assert(ALIBI || !CAP, "the soft-clamp forms are the ALiBi-capable ones");
  constexpr int KS = DH / 4, ND = DH / 16, KST = DH + 2;
  __shared__ float Ks[TK][KST], Vs[TK][KST];
  __shared__ float Ps[4][16][PST];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x;
  const int bh = blockIdx.y, b = bh / a.H, ns = a.n;
  const int q0 = blockIdx.x * TQ;
  const int len = a.lens[b];
  const int n = a.ep_off ? min(len, ns) : ns;   // packed rows: the episode's own length
  const int h = bh - b * a.H;
  if (q0 >= n) return;   // (packed rows: a query tile past the episode; workgroup-uniform)
  const int64_t ib = ebase(a, a.in, b) + h * a.in.sh, ob = ebase(a, a.out, b) + h * a.out.sh;
  const int isi = a.in.si, osi = a.out.si;
  const int64_t kb = GQA ? ebase(a, a.kv, b) + kv_head_of(h, a.Hkv) * a.kv.sh : ib;
  const int ksi = GQA ? a.kv.si : isi;
  const int lr = lane & 15, lg = lane >> 4;
  const uint32_t off = a.offset + (uint32_t)bh;
  const float slope = ALIBI ? ((CAP && !a.alibi) ? 0.f : a.alibi[h]) : 0.f;

  float qa[KS];
  {
    const int i = q0 + 16 * w + lr;
#pragma unroll
    for (int s = 0; s < KS; ++s) qa[s] = (i < n) ? a.Q[ib + (int64_t)i * isi + 4 * s + lg] : 0.f;
  }
  float m[4], l[4];
  f32x4v o[ND];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
#pragma unroll
  for (int d = 0; d < ND; ++d) o[d] = f32x4v{0.f, 0.f, 0.f, 0.f};

  if constexpr (SINK) {
    if (a.Z) {   // the zero key: score 0, value 0
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        m[r] = 0.f;
        l[r] = 1.f;
      }
    }
    if (a.M > 0) {   // the memory rows of this head's kv head: one 16-column sub-tile (columns >= M masked)
      const float* mk = a.MK + (int64_t)kv_head_of(h, a.Hkv) * a.M * DH;
      const float* mv = a.MV + (int64_t)kv_head_of(h, a.Hkv) * a.M * DH;
      for (int x = tid; x < 16 * DH; x += 256) {
        const int j = x / DH, c = x - j * DH;
        Ks[j][c] = j < a.M ? mk[j * DH + c] : 0.f;
        Vs[j][c] = j < a.M ? mv[j * DH + c] : 0.f;
      }
      __syncthreads();
      f32x4v sacc = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) sacc = mfma16(qa[s], Ks[lr][4 * s + lg], sacc);
      u32x4_t kw = {};
      if (a.thresh) kw = philox4x32_10((uint32_t)((q0 + 16 * w + 4 * lg) >> 2), SINK_C1 | (uint32_t)lr, off, a.c3, a.seed);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float ms = sacc[r] * a.scale;
        if constexpr (CAP) ms = a.cap * tanhf(ms * a.inv_cap);
        const float sv = lr < a.M ? ms : -INFINITY;
        float mx = sv;
#pragma unroll
        for (int o2 = 1; o2 < 16; o2 <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
        const float mnew = fmaxf(m[r], mx);
        const float alpha = (m[r] == -INFINITY) ? 0.f : expf(m[r] - mnew);
        const float p = (sv == -INFINITY) ? 0.f : expf(sv - mnew);
        float rs = p;
#pragma unroll
        for (int o2 = 1; o2 < 16; o2 <<= 1) rs += __shfl_xor(rs, o2, 64);
        Ps[w][4 * lg + r][lr] = (a.thresh && qword(kw, r) < a.thresh) ? 0.f : p * a.inv_keep;
        l[r] = l[r] * alpha + rs;
        m[r] = mnew;
      }
      wave_sync();
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int s = 0; s < 4; ++s) o[d] = mfma16(Ps[w][lr][4 * s + lg], Vs[4 * s + lg][16 * d + lr], o[d]);
      wave_sync();
    }
  }
  const int last_key = min(min(a.causal ? q0 + TQ - 1 : n - 1, n - 1), len - 1);
  // the first key tile of the band: row q0's oldest visible key q0 - W.  A later row of the tile may
  // see nothing in it (its band starts in the next tile): it carries m = -inf, l = 0, o = 0 on
  // (alpha and p below are 0 then: no exp(-inf + inf))
  for (int kt = max(0, q0 - a.window) / TK; kt * TK <= last_key; ++kt) {
    __syncthreads();
    for (int x = tid; x < TK * DH; x += 256) {
      const int j = x / DH, c = x - j * DH, jj = kt * TK + j;
      Ks[j][c] = jj < n ? a.K[kb + (int64_t)jj * ksi + c] : 0.f;
      Vs[j][c] = jj < n ? a.V[kb + (int64_t)jj * ksi + c] : 0.f;
    }
    __syncthreads();
    f32x4v sacc[4];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      sacc[sub] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) sacc[sub] = mfma16(qa[s], Ks[16 * sub + lr][4 * s + lg], sacc[sub]);
    }
    // keep words: this lane's rows q0 + 16 w + 4 lg + 0..3 share one Philox block per key column
    // (word = row & 3), so one block per column instead of one per element
    u32x4_t kws[4] = {};
    if (a.thresh8) {   // byte mode: one block holds all 16 keep bytes of this lane's scores
      kws[0] = philox4x32_10((uint32_t)((q0 + 16 * w + 4 * lg) >> 2), (uint32_t)(kt * 16 + lr), off, a.c3, a.seed);
    } else if (a.thresh) {
#pragma unroll
      for (int sub = 0; sub < 4; ++sub)
        kws[sub] = philox4x32_10((uint32_t)((q0 + 16 * w + 4 * lg) >> 2), (uint32_t)(kt * TK + 16 * sub + lr), off,
                                 a.c3, a.seed);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = q0 + 16 * w + 4 * lg + r;
      float sv[4];
      float mx = -INFINITY;
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        const int j = kt * TK + 16 * sub + lr;
        const bool ok = (j <= i || !a.causal) && (j < len) && (i - j <= a.window);
        float sc = sacc[sub][r] * a.scale;
        if constexpr (ALIBI) sc -= slope * (float)(i - j);
        if constexpr (CAP) sc = a.cap * tanhf(sc * a.inv_cap);
        sv[sub] = ok ? sc : -INFINITY;
        mx = fmaxf(mx, sv[sub]);
      }
#pragma unroll
      for (int o2 = 1; o2 < 16; o2 <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
      const float mnew = fmaxf(m[r], mx);
      const float alpha = (m[r] == -INFINITY) ? 0.f : expf(m[r] - mnew);
      float rs = 0.f;
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        const float p = (sv[sub] == -INFINITY) ? 0.f : expf(sv[sub] - mnew);
        rs += p;
        float pd = p;
        if (a.thresh8) pd = (qbyte(kws[0], sub, r) >= a.thresh8) ? p * a.inv_keep : 0.f;
        else if (a.thresh) pd = (qword(kws[sub], r) >= a.thresh) ? p * a.inv_keep : 0.f;
        Ps[w][4 * lg + r][16 * sub + lr] = pd;
      }
#pragma unroll
      for (int o2 = 1; o2 < 16; o2 <<= 1) rs += __shfl_xor(rs, o2, 64);
      l[r] = l[r] * alpha + rs;
      m[r] = mnew;
#pragma unroll
      for (int d = 0; d < ND; ++d) o[d][r] *= alpha;
    }
    wave_sync();
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
      for (int s = 0; s < TK / 4; ++s) o[d] = mfma16(Ps[w][lr][4 * s + lg], Vs[4 * s + lg][16 * d + lr], o[d]);
    wave_sync();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 16 * w + 4 * lg + r;
    if (i < n) {
      // a padded row (i >= len) whose whole band lies past the valid keys saw nothing: o = 0, lse = 0
      // here; k_attn_dead_fwd then stores its uniform average (no window: every row of an episode
      // with a valid key sees key 0)
      const bool dead = !SINK && a.window != NO_WINDOW && l[r] == 0.f;   // (with a sink l >= its term > 0)
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const int64_t at = ob + (int64_t)i * osi + 16 * d + lr;
        const float ov = dead ? 0.f : o[d][r] / l[r];
        a.Oout[at] = ov;
        if (a.OGout)   // gated values (x-transformers attn_gate_values)
          a.OGout[at] = ov * sigmoidf_(a.G[ebase(a, a.gate, b) + h * a.gate.sh + (int64_t)i * a.gate.si + 16 * d + lr]);
      }
      if (lr == 0) a.LSEout[(int64_t)bh * ns + i] = dead ? 0.f : m[r] + logf(l[r]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// DQ (long episodes, n > FB_MAXN): the dQ kernel's pass is folded in as in k_attn_bwd_fused — per
// (key tile, query tile) pair, once the four waves' dS images are in LDS, wave w multiplies its 16
// query rows of dS by the key tile (staged once per workgroup) — but the key tiles stay spread over
// the grid: a query row whose only contributing key tile is tile 0 (query tile 0, or an episode of
// <= 64 steps: min(qt, (len - 1) / 64) = 0) gets dQ written here, bit-identical to k_attn_bwd_dq;
// the other rows get one partial per contributing key tile in dQp, summed in ascending key-tile
// order by k_attn_dq_reduce.  (141 registers, 3 waves per SIMD: held to 128 it spilled 12.)
// With a window W the contributing key tiles of query tile qt are max(0, 64 qt - W) / 64 ..
// min(qt, (len - 1) / 64): one tile -> dQ directly, several -> partials, none (padded rows past the
// band) -> the reduce stores 0.
// WIN = false (dh = 16 without a window, the C2 / C3 shapes): the window tests are compiled out — with
// them the 128-register budget of the 4-waves-per-SIMD form spilled 2 registers; every other form
// takes the window at run time (NO_WINDOW: none)
// GQA = true (Hkv < H, always with WIN): the grid is (key tile, b Hkv); the workgroup holds its kv
// head's key tile and walks the query heads h of the group (kv_head_of(h, Hkv) == its kv head) in
// ascending order, each over its query tiles as before, adding into the same dK / dV registers — a
// fixed summation order, no atomics.  D, the dQ partials and the keep bits stay per query head.
// GQA = false: one pass with h = the grid's head, the code of before
// ALIBI = true (always with GQA, Hkv = H included): p is recomputed with the query head's distance penalty
// CAP = true (always with ALIBI; the slope is 0 when a.alibi is NULL): p is recomputed from cap tanh(score /
// cap) and the dS image that feeds dK (and the folded dQ) carries the factor 1 - tanh^2; dV takes P~ as before
template <int DH, bool DQ = false, bool WIN = true, bool GQA = false, bool ALIBI = false, bool CAP = false>
__global__ __launch_bounds__(256, DH == 16 ? ((DQ || WIN) ? 3 : 4) : 1) void k_attn_bwd_dkdv(const AttnArgs a) {
  static_assert(WIN || !GQA, "the GQA forms take the window at run time");
  static_assert(GQA || !ALIBI, "the ALiBi forms take the kv head mapping at run time");
  static_assert(ALIBI || !CAP, "the soft-clamp forms are the ALiBi-capable ones");
  constexpr int KS = DH / 4, ND = DH / 16, KST = DH + 2;
  __shared__ float Qs[TQ][KST], dOs[TQ][KST];
  __shared__ float Ks[DQ ? TK : 1][KST];
  __shared__ float Ls[TQ], Dls[TQ];
  // one per-wave tile image, used for P~ (dV) and then for dS (dK): 26.6 KB of LDS per workgroup,
  // six resident per CU; at dh = 16 the register budget is held to 128 (4 waves per SIMD: 168 gave
  // 3, and a quarter of the C3 grid ran as a second round), so the C3 grid is one round
  __shared__ float Ps[4][16][PST];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x;
  // the grid's head hk: the kv head (GQA) or the query head, which is its own kv head
  const int nhk = GQA ? a.Hkv : a.H;
  const int b = blockIdx.y / nhk, ns = a.n;
  const int j0 = blockIdx.x * TK;
  const int len = a.lens[b];
  const int n = a.ep_off ? min(len, ns) : ns;   // packed rows: the episode's own length
  const int hk = blockIdx.y - b * nhk;
  // the query head at work: the grid's own (GQA: set per pass of the group loop below)
  int bh = blockIdx.y, h = hk;
  int64_t ib = ebase(a, a.in, b) + h * a.in.sh, ob = ebase(a, a.out, b) + h * a.out.sh, gb = ebase(a, a.grad, b) + h * a.grad.sh;
  const int isi = a.in.si, osi = a.out.si, gsi = a.grad.si;
  const int lr = lane & 15, lg = lane >> 4;
  uint32_t off = a.offset + (uint32_t)bh;
  // K, V and dK, dV of head hk (GQA: in their own layouts)
  const int64_t kb = GQA ? ebase(a, a.kv, b) + hk * a.kv.sh : ib;
  const int64_t kgb = GQA ? ebase(a, a.kvgrad, b) + hk * a.kvgrad.sh : gb;
  const int ksi = GQA ? a.kv.si : isi, kgsi = GQA ? a.kvgrad.si : gsi;

  float ka[KS], va[KS];
  {
    const int j = j0 + 16 * w + lr;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      ka[s] = (j < n) ? a.K[kb + (int64_t)j * ksi + 4 * s + lg] : 0.f;
      va[s] = (j < n) ? a.V[kb + (int64_t)j * ksi + 4 * s + lg] : 0.f;
    }
  }
  f32x4v dk[ND], dv[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    dk[d] = f32x4v{0.f, 0.f, 0.f, 0.f};
    dv[d] = f32x4v{0.f, 0.f, 0.f, 0.f};
  }
  const int kmax = len > 0 ? (len - 1) / TK : 0;   // DQ: the last key tile holding a valid key
  if constexpr (DQ) {
    for (int x = tid; x < TK * DH; x += 256) {
      const int j = x / DH, c = x - j * DH, jj = j0 + j;
      Ks[j][c] = jj < n ? a.K[kb + (int64_t)jj * ksi + c] : 0.f;
    }
    if (!GQA && j0 == 0 && len <= 0) {   // no valid key: the rows' dQ is 0, this workgroup its only writer
      for (int x = tid; x < n * DH; x += 256) {
        const int i = x / DH, c = x - i * DH;
        a.dQ[gb + (int64_t)i * gsi + c] = 0.f;
      }
    }
  }
  float slope = 0.f;   // ALIBI: the query head's, set per pass of the group loop
  int g = 0;   // GQA: the query heads, ascending; one pass each for those of this kv head
  do {
    if constexpr (GQA) {
      while (g < a.H && kv_head_of(g, a.Hkv) != hk) ++g;   // (workgroup-uniform) the next query head of kv head hk
      if (g >= a.H) break;
      h = g;
      bh = b * a.H + h;
      ib = ebase(a, a.in, b) + h * a.in.sh, ob = ebase(a, a.out, b) + h * a.out.sh, gb = ebase(a, a.grad, b) + h * a.grad.sh;
      off = a.offset + (uint32_t)bh;
      if constexpr (ALIBI) slope = (CAP && !a.alibi) ? 0.f : a.alibi[h];
      if (DQ && j0 == 0 && len <= 0) {   // (as above, per query head)
        for (int x = tid; x < n * DH; x += 256) {
          const int i = x / DH, c = x - i * DH;
          a.dQ[gb + (int64_t)i * gsi + c] = 0.f;
        }
      }
    }
    // a key tile without a valid key (a tile of padded rows) under WIN: its workgroup still owns the D
    // of its own query tile — it stages that one tile, stores D (the very same sum) and stops there
    // (without a window the key-tile-0 workgroup visits every query tile and stays the owner, as it
    // always was: no extra staging)
    const bool live = j0 < len;
    const bool own0 = !WIN || a.window == NO_WINDOW;
    if (live || (!own0 && len > 0)) {
      // query tiles of the band: from the diagonal to the last one holding a row <= j0 + TK - 1 + W
      const int n_end = !WIN ? n : (live ? min(n, j0 + TK + a.window) : min(n, j0 + TQ));
      for (int qt = j0 / TQ; qt * TQ < n_end; ++qt) {
        __syncthreads();
        for (int x = tid; x < TQ * DH; x += 256) {
          const int i = x / DH, c = x - i * DH, ii = qt * TQ + i;
          Qs[i][c] = ii < n ? a.Q[ib + (int64_t)ii * isi + c] : 0.f;
          dOs[i][c] = ii < n ? a.dO[ob + (int64_t)ii * osi + c] : 0.f;
        }
        // D_i = rowsum(dO_i * O_i) of the tile's query rows, computed here (the O row in registers
        // while the tile stages) in the order of a sequential sum over the head dimension; the
        // diagonal workgroup (key tile == query tile: a row always sees itself, so a window never
        // skips the pair) stores it for k_attn_bwd_dq
        float orow[DH];
        if (tid < TQ) {
          const int ii = qt * TQ + tid;
          Ls[tid] = ii < n ? a.LSE[(int64_t)bh * ns + ii] : 0.f;
#pragma unroll
          for (int c = 0; c < DH; ++c) orow[c] = ii < n ? a.O[ob + (int64_t)ii * osi + c] : 0.f;
        }
        __syncthreads();
        if (tid < TQ) {
          const int ii = qt * TQ + tid;
          float dsum = 0.f;
#pragma unroll
          for (int c = 0; c < DH; ++c) dsum += dOs[tid][c] * orow[c];
          Dls[tid] = dsum;
          if ((own0 ? j0 == 0 : qt * TQ == j0) && ii < n) a.Dout[(int64_t)bh * ns + ii] = dsum;
        }
        if (WIN && !live) break;   // (workgroup-uniform)
        __syncthreads();
        float dsr[4][4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
          f32x4v st = f32x4v{0.f, 0.f, 0.f, 0.f}, dpt = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            st = mfma16(ka[s], Qs[16 * sub + lr][4 * s + lg], st);
            dpt = mfma16(va[s], dOs[16 * sub + lr][4 * s + lg], dpt);
          }
          const int il = 16 * sub + lr, i = qt * TQ + il;
          // keep words of row i at key columns j0 + 16 w + 4 lg + 0..3: the four lanes of a quad hold
          // rows 4 (i >> 2) + 0..3; lane c computes the block of column 4 lg + c (its four words are
          // the quad's four rows) and a quad transpose hands every lane its row's word of each column
          // (byte mode: lane c computes the block of column class 4 lg + c, takes word w — this wave's
          // 16-column group — and the quad transpose deals byte (row & 3) of each column's word)
          uint32_t kq[4] = {0u, 0u, 0u, 0u};
          if (a.thresh8) {
            const u32x4_t kb = philox4x32_10((uint32_t)(i >> 2), (uint32_t)((j0 >> 6) * 16 + 4 * lg + (lr & 3)), off,
                                             a.c3, a.seed);
            const uint32_t wd = qword(kb, w);
#pragma unroll
            for (int c = 0; c < 4; ++c) kq[c] = (wd >> (8 * c)) & 0xFFu;
            quad_transpose(kq, lane);
          } else if (a.thresh) {
            const u32x4_t kb = philox4x32_10((uint32_t)(i >> 2), (uint32_t)(j0 + 16 * w + 4 * lg + (lr & 3)), off,
                                             a.c3, a.seed);
            kq[0] = kb.x;
            kq[1] = kb.y;
            kq[2] = kb.z;
            kq[3] = kb.w;
            quad_transpose(kq, lane);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = j0 + 16 * w + 4 * lg + r;
            // 0 <= i - j <= W in one compare
            const bool ok = (WIN ? (unsigned)(i - j) <= (unsigned)a.window : j <= i) && (j < len) && (i < n);
            float sc = st[r] * a.scale;
            if constexpr (ALIBI) sc -= slope * (float)(i - j);
            float dt = 1.f;   // CAP: d s / d x = 1 - tanh^2(x / cap)
            if constexpr (CAP) {
              const float t = tanhf(sc * a.inv_cap);
              sc = a.cap * t;
              dt = 1.f - t * t;
            }
            const float p = ok ? expf(sc - Ls[il]) : 0.f;
            float z = 1.f;
            if (a.thresh8 && ok) z = (kq[r] >= a.thresh8) ? a.inv_keep : 0.f;
            else if (a.thresh && ok) z = (kq[r] >= a.thresh) ? a.inv_keep : 0.f;
            Ps[w][4 * lg + r][il] = p * z;
            dsr[sub][r] = CAP ? p * (dpt[r] * z - Dls[il]) * dt : p * (dpt[r] * z - Dls[il]);
          }
        }
        wave_sync();
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
          for (int s = 0; s < TQ / 4; ++s) dv[d] = mfma16(Ps[w][lr][4 * s + lg], dOs[4 * s + lg][16 * d + lr], dv[d]);
        wave_sync();
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
          for (int r = 0; r < 4; ++r) Ps[w][4 * lg + r][16 * sub + lr] = dsr[sub][r];
        wave_sync();
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
          for (int s = 0; s < TQ / 4; ++s) dk[d] = mfma16(Ps[w][lr][4 * s + lg], Qs[4 * s + lg][16 * d + lr], dk[d]);
        if constexpr (DQ) {
          __syncthreads();   // every wave's dS image of the pair is in LDS
          // dQ rows 16 w .. 16 w + 15 of this query tile: dS[query][key] = image [key / 16][key % 16][query]
          f32x4v dq[ND];
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            dq[d] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < TK / 4; ++s) {
              const int j = 4 * s + lg;
              dq[d] = mfma16(Ps[j >> 4][j & 15][16 * w + lr], Ks[j][16 * d + lr], dq[d]);
            }
          }
          // the key tiles visiting this query tile: max(0, qt TQ - W) / TK .. min(qt, kmax); one: dQ directly
          const bool sole = (WIN ? max(0, qt * TQ - a.window) / TK : 0) == min(qt, kmax);
          const int64_t BH = GQA ? (int64_t)(gridDim.y / nhk) * a.H : (int64_t)gridDim.y;   // b H: the partials are per query head
          const int64_t pb = ((int64_t)blockIdx.x * BH + bh) * ns;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = qt * TQ + 16 * w + 4 * lg + r;
            if (i < n) {
#pragma unroll
              for (int d = 0; d < ND; ++d) {
                if (sole) a.dQ[gb + (int64_t)i * gsi + 16 * d + lr] = dq[d][r] * a.scale;
                else a.dQp[(pb + i) * DH + 16 * d + lr] = dq[d][r];
              }
            }
          }
        } else {
          wave_sync();
        }
      }
    }
  } while (GQA && ++g < a.H);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + 16 * w + 4 * lg + r;
    if (j < n) {
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        a.dK[kgb + (int64_t)j * kgsi + 16 * d + lr] = dk[d][r] * a.scale;
        a.dV[kgb + (int64_t)j * kgsi + 16 * d + lr] = dv[d][r];
      }
    }
  }
}

// dQ of the rows with more than one contributing key tile: the partials of key tiles
// max(0, qt 64 - W) / 64 .. min(qt, (len - 1) / 64) — exactly the tiles that wrote one — summed in
// ascending order (k_attn_bwd_dkdv<DH, true>); thread per (row, 4 channels)
template <int DH>
__global__ __launch_bounds__(256) void k_attn_dq_reduce(const AttnArgs a, int BH) {
  constexpr int C4 = DH / 4;
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int ns = a.n;
  if (x >= (int64_t)BH * ns * C4) return;
  const int c4 = (int)(x % C4);
  const int64_t row = x / C4;
  const int bh = (int)(row / ns), i = (int)(row - (int64_t)bh * ns);
  const int b = bh / a.H, h = bh - b * a.H;
  const int len = a.lens[b];
  if (a.ep_off && i >= min(len, ns)) return;   // packed rows: past the episode's own length
  if (len <= 0) return;   // zero-filled by the key-tile-0 workgroup
  const int qt = i / TQ;
  const int m = min(qt, (len - 1) / TK), f = max(0, qt * TQ - a.window) / TK;
  if (m == f) return;   // one key tile visits the row's query tile: written by it
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);   // f > m: none does (padded rows past the band): dQ = 0
  if (f < m) acc = *reinterpret_cast<const float4*>(a.dQp + (((int64_t)f * BH + bh) * ns + i) * DH + 4 * c4);
  for (int kt = f + 1; kt <= m; ++kt) {
    const float4 p = *reinterpret_cast<const float4*>(a.dQp + (((int64_t)kt * BH + bh) * ns + i) * DH + 4 * c4);
    acc.x += p.x;
    acc.y += p.y;
    acc.z += p.z;
    acc.w += p.w;
  }
  float* dst = a.dQ + ebase(a, a.grad, b) + h * a.grad.sh + (int64_t)i * a.grad.si + 4 * c4;
  dst[0] = acc.x * a.scale;
  dst[1] = acc.y * a.scale;
  dst[2] = acc.z * a.scale;
  dst[3] = acc.w * a.scale;
}

// ---------------------------------------------------------------------------------------------
// ALIBI, CAP: as k_attn_bwd_dkdv (ALIBI always with GQA, CAP always with ALIBI)
template <int DH, bool GQA = false, bool ALIBI = false, bool CAP = false>
__global__ __launch_bounds__(256) void k_attn_bwd_dq(const AttnArgs a) {
  static_assert(GQA || !ALIBI, "the ALiBi forms take the kv head mapping at run time");
  static_assert(ALIBI || !CAP, "the soft-clamp forms are the ALiBi-capable ones");
  constexpr int KS = DH / 4, ND = DH / 16, KST = DH + 2;
  __shared__ float Ks[TK][KST], Vs[TK][KST];
  __shared__ float Ds[4][16][PST];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x;
  const int bh = blockIdx.y, b = bh / a.H, ns = a.n;
  const int q0 = blockIdx.x * TQ;
  const int len = a.lens[b];
  const int n = a.ep_off ? min(len, ns) : ns;   // packed rows: the episode's own length
  const int h = bh - b * a.H;
  if (q0 >= n) return;   // (packed rows: a query tile past the episode; workgroup-uniform)
  const int64_t ib = ebase(a, a.in, b) + h * a.in.sh, ob = ebase(a, a.out, b) + h * a.out.sh, gb = ebase(a, a.grad, b) + h * a.grad.sh;
  const int isi = a.in.si, osi = a.out.si, gsi = a.grad.si;
  const int64_t kb = GQA ? ebase(a, a.kv, b) + kv_head_of(h, a.Hkv) * a.kv.sh : ib;   // the kv head's K / V
  const int ksi = GQA ? a.kv.si : isi;
  const int lr = lane & 15, lg = lane >> 4;
  const uint32_t off = a.offset + (uint32_t)bh;
  const float slope = ALIBI ? ((CAP && !a.alibi) ? 0.f : a.alibi[h]) : 0.f;

  float qa[KS], da[KS];
  {
    const int i = q0 + 16 * w + lr;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qa[s] = (i < n) ? a.Q[ib + (int64_t)i * isi + 4 * s + lg] : 0.f;
      da[s] = (i < n) ? a.dO[ob + (int64_t)i * osi + 4 * s + lg] : 0.f;
    }
  }
  float lse[4], dl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 16 * w + 4 * lg + r;
    lse[r] = i < n ? a.LSE[(int64_t)bh * ns + i] : 0.f;
    dl[r] = i < n ? a.Dl[(int64_t)bh * ns + i] : 0.f;
  }
  f32x4v dq[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) dq[d] = f32x4v{0.f, 0.f, 0.f, 0.f};
  const int last_key = min(min(a.causal ? q0 + TQ - 1 : n - 1, n - 1), len - 1);
  for (int kt = max(0, q0 - a.window) / TK; kt * TK <= last_key; ++kt) {   // the band's key tiles
    __syncthreads();
    for (int x = tid; x < TK * DH; x += 256) {
      const int j = x / DH, c = x - j * DH, jj = kt * TK + j;
      Ks[j][c] = jj < n ? a.K[kb + (int64_t)jj * ksi + c] : 0.f;
      Vs[j][c] = jj < n ? a.V[kb + (int64_t)jj * ksi + c] : 0.f;
    }
    __syncthreads();
    // byte mode: one block per lane and key tile holds all 16 keep bytes of its scores
    const u32x4_t kb8 = a.thresh8 ? philox4x32_10((uint32_t)((q0 + 16 * w + 4 * lg) >> 2), (uint32_t)(kt * 16 + lr),
                                                  off, a.c3, a.seed)
                                  : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      f32x4v s_ = f32x4v{0.f, 0.f, 0.f, 0.f}, dp = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        s_ = mfma16(qa[s], Ks[16 * sub + lr][4 * s + lg], s_);
        dp = mfma16(da[s], Vs[16 * sub + lr][4 * s + lg], dp);
      }
      const int jl = 16 * sub + lr, j = kt * TK + jl;
      // this lane's rows q0 + 16 w + 4 lg + 0..3 share one Philox block (word = row & 3)
      const u32x4_t kw = (a.thresh && !a.thresh8) ? philox4x32_10((uint32_t)((q0 + 16 * w + 4 * lg) >> 2), (uint32_t)j,
                                                                  off, a.c3, a.seed)
                                                  : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + 16 * w + 4 * lg + r;
        const bool ok = ((unsigned)(i - j) <= (unsigned)a.window) && (j < len) && (i < n);   // 0 <= i - j <= W
        float sc = s_[r] * a.scale;
        if constexpr (ALIBI) sc -= slope * (float)(i - j);
        float dt = 1.f;   // CAP: d s / d x = 1 - tanh^2(x / cap)
        if constexpr (CAP) {
          const float t = tanhf(sc * a.inv_cap);
          sc = a.cap * t;
          dt = 1.f - t * t;
        }
        const float p = ok ? expf(sc - lse[r]) : 0.f;
        float z = 1.f;
        if (a.thresh8 && ok) z = (qbyte(kb8, sub, r) >= a.thresh8) ? a.inv_keep : 0.f;
        else if (a.thresh && ok) z = (qword(kw, r) >= a.thresh) ? a.inv_keep : 0.f;
        Ds[w][4 * lg + r][jl] = CAP ? p * (dp[r] * z - dl[r]) * dt : p * (dp[r] * z - dl[r]);
      }
    }
    wave_sync();
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
      for (int s = 0; s < TK / 4; ++s) dq[d] = mfma16(Ds[w][lr][4 * s + lg], Ks[4 * s + lg][16 * d + lr], dq[d]);
    wave_sync();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 16 * w + 4 * lg + r;
    if (i < n) {
#pragma unroll
      for (int d = 0; d < ND; ++d) a.dQ[gb + (int64_t)i * gsi + 16 * d + lr] = dq[d][r] * a.scale;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Fused backward for short episodes (n <= FB_MAXN, dh = 16): one workgroup per (episode, head)
// walks its key tiles; per (key tile, query tile) pair it forms P, P~ and dS ONCE and takes dV, dK
// (as k_attn_bwd_dkdv) and dQ from them — the dQ kernel's second pass over the same pairs (scores,
// softmax, keep bits and dP recomputed) is gone.  dQ: after the four waves' dS images of the pair are
// in LDS, wave w multiplies rows 16 w .. 16 w + 15 of dS (queries) by the key tile (staged in LDS)
// into its register accumulator of that query tile; the pairs are visited in (key tile, query tile)
// order, the same for every workgroup (deterministic).  Keep bits, masks and D = rowsum(dO * O) as
// k_attn_bwd_dkdv (bit-identical dK / dV; dQ sums key tiles in ascending order like k_attn_bwd_dq).
constexpr int FB_MAXN = 128, FB_QT = FB_MAXN / TQ;
template <int DH>
__global__ __launch_bounds__(256) void k_attn_bwd_fused(const AttnArgs a) {
  constexpr int KS = DH / 4, ND = DH / 16, KST = DH + 2;
  __shared__ float Qs[TQ][KST], dOs[TQ][KST], Ks[TK][KST];
  __shared__ float Ls[TQ], Dls[TQ];
  __shared__ float Ps[4][16][PST];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x;
  const int bh = blockIdx.x, b = bh / a.H, ns = a.n;
  const int len = a.lens[b];
  const int n = a.ep_off ? min(len, ns) : ns;   // packed rows: the episode's own length
  const int h = bh - b * a.H;
  const int64_t ib = ebase(a, a.in, b) + h * a.in.sh, ob = ebase(a, a.out, b) + h * a.out.sh, gb = ebase(a, a.grad, b) + h * a.grad.sh;
  const int isi = a.in.si, osi = a.out.si, gsi = a.grad.si;
  const int lr = lane & 15, lg = lane >> 4;
  const uint32_t off = a.offset + (uint32_t)bh;
  const int nq = (n + TQ - 1) / TQ;

  f32x4v dq[FB_QT][ND];
#pragma unroll
  for (int q = 0; q < FB_QT; ++q)
#pragma unroll
    for (int d = 0; d < ND; ++d) dq[q][d] = f32x4v{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < nq; ++kt) {
    const int j0 = kt * TK;
    float ka[KS], va[KS];
    {
      const int j = j0 + 16 * w + lr;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        ka[s] = (j < n) ? a.K[ib + (int64_t)j * isi + 4 * s + lg] : 0.f;
        va[s] = (j < n) ? a.V[ib + (int64_t)j * isi + 4 * s + lg] : 0.f;
      }
    }
    f32x4v dk[ND], dv[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      dk[d] = f32x4v{0.f, 0.f, 0.f, 0.f};
      dv[d] = f32x4v{0.f, 0.f, 0.f, 0.f};
    }
    const bool live = j0 < len;   // (else, with a window and a valid key in the episode: only D of the diagonal tile, as k_attn_bwd_dkdv)
    const bool own0 = a.window == NO_WINDOW;   // no window: key tile 0 visits every query tile and owns D
    if (live || (!own0 && len > 0)) {
#pragma unroll
      for (int qt = 0; qt < FB_QT; ++qt) {
        if (qt < kt || qt >= nq) continue;   // (workgroup-uniform) causal: query tiles from the key tile on
        if (!live && qt != kt) continue;
        if (qt * TQ - (j0 + TK - 1) > a.window) continue;   // (workgroup-uniform) the pair lies outside the band
        __syncthreads();
        for (int x = tid; x < TQ * DH; x += 256) {
          const int i = x / DH, c = x - i * DH, ii = qt * TQ + i, jj = j0 + i;
          Qs[i][c] = ii < n ? a.Q[ib + (int64_t)ii * isi + c] : 0.f;
          dOs[i][c] = ii < n ? a.dO[ob + (int64_t)ii * osi + c] : 0.f;
          Ks[i][c] = jj < n ? a.K[ib + (int64_t)jj * isi + c] : 0.f;
        }
        float orow[DH];
        if (tid < TQ) {
          const int ii = qt * TQ + tid;
          Ls[tid] = ii < n ? a.LSE[(int64_t)bh * ns + ii] : 0.f;
#pragma unroll
          for (int c = 0; c < DH; ++c) orow[c] = ii < n ? a.O[ob + (int64_t)ii * osi + c] : 0.f;
        }
        __syncthreads();
        if (tid < TQ) {
          float dsum = 0.f;
#pragma unroll
          for (int c = 0; c < DH; ++c) dsum += dOs[tid][c] * orow[c];
          Dls[tid] = dsum;
          const int ii = qt * TQ + tid;
          if ((own0 ? kt == 0 : kt == qt) && ii < n) a.Dout[(int64_t)bh * ns + ii] = dsum;   // as k_attn_bwd_dkdv
        }
        if (!live) continue;   // (workgroup-uniform)
        __syncthreads();
        float dsr[4][4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
          f32x4v st = f32x4v{0.f, 0.f, 0.f, 0.f}, dpt = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            st = mfma16(ka[s], Qs[16 * sub + lr][4 * s + lg], st);
            dpt = mfma16(va[s], dOs[16 * sub + lr][4 * s + lg], dpt);
          }
          const int il = 16 * sub + lr, i = qt * TQ + il;
          uint32_t kq[4] = {0u, 0u, 0u, 0u};
          if (a.thresh8) {
            const u32x4_t kb = philox4x32_10((uint32_t)(i >> 2), (uint32_t)((j0 >> 6) * 16 + 4 * lg + (lr & 3)), off,
                                             a.c3, a.seed);
            const uint32_t wd = qword(kb, w);
#pragma unroll
            for (int c = 0; c < 4; ++c) kq[c] = (wd >> (8 * c)) & 0xFFu;
            quad_transpose(kq, lane);
          } else if (a.thresh) {
            const u32x4_t kb = philox4x32_10((uint32_t)(i >> 2), (uint32_t)(j0 + 16 * w + 4 * lg + (lr & 3)), off,
                                             a.c3, a.seed);
            kq[0] = kb.x;
            kq[1] = kb.y;
            kq[2] = kb.z;
            kq[3] = kb.w;
            quad_transpose(kq, lane);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = j0 + 16 * w + 4 * lg + r;
            const bool ok = ((unsigned)(i - j) <= (unsigned)a.window) && (j < len) && (i < n);   // 0 <= i - j <= W
            const float p = ok ? expf(st[r] * a.scale - Ls[il]) : 0.f;
            float z = 1.f;
            if (a.thresh8 && ok) z = (kq[r] >= a.thresh8) ? a.inv_keep : 0.f;
            else if (a.thresh && ok) z = (kq[r] >= a.thresh) ? a.inv_keep : 0.f;
            Ps[w][4 * lg + r][il] = p * z;
            dsr[sub][r] = p * (dpt[r] * z - Dls[il]);
          }
        }
        wave_sync();
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
          for (int s = 0; s < TQ / 4; ++s) dv[d] = mfma16(Ps[w][lr][4 * s + lg], dOs[4 * s + lg][16 * d + lr], dv[d]);
        wave_sync();
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
          for (int r = 0; r < 4; ++r) Ps[w][4 * lg + r][16 * sub + lr] = dsr[sub][r];
        wave_sync();
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
          for (int s = 0; s < TQ / 4; ++s) dk[d] = mfma16(Ps[w][lr][4 * s + lg], Qs[4 * s + lg][16 * d + lr], dk[d]);
        __syncthreads();   // every wave's dS image of the pair is in LDS
        // dQ rows 16 w .. 16 w + 15 of this query tile: dS[query][key] = image [key / 16][key % 16][query]
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
          for (int s = 0; s < TK / 4; ++s) {
            const int j = 4 * s + lg;
            dq[qt][d] = mfma16(Ps[j >> 4][j & 15][16 * w + lr], Ks[j][16 * d + lr], dq[qt][d]);
          }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + 16 * w + 4 * lg + r;
      if (j < n) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          a.dK[gb + (int64_t)j * gsi + 16 * d + lr] = dk[d][r] * a.scale;
          a.dV[gb + (int64_t)j * gsi + 16 * d + lr] = dv[d][r];
        }
      }
    }
  }
#pragma unroll
  for (int qt = 0; qt < FB_QT; ++qt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = qt * TQ + 16 * w + 4 * lg + r;
      if (qt < nq && i < n) {
#pragma unroll
        for (int d = 0; d < ND; ++d) a.dQ[gb + (int64_t)i * gsi + 16 * d + lr] = dq[qt][d][r] * a.scale;
      }
    }
}

// ---------------------------------------------------------------------------------------------
// Rows that see no key under a window: the padded rows i >= len + W of the padded layout.
// x-transformers fills masked scores with the finite -max, so such a row's softmax is uniform over
// all n key positions (future and padded ones included), p_ij = 1 / n, and no gradient reaches its
// scores.  They are padded tokens, but the scalar HL-Gauss mean puts them into the critic loss, so
// they are reproduced.  The flash kernels leave these rows at o = 0 (dQ, dK contributions 0); these
// two launches add the uniform part:
//   forward   o_i = sum_j z_ij v_j / n (and its gated copy)
//   backward  dv_j += sum_{dead i} z_ij do_i / n
// z_ij: the dropout keep factor of the same absolute (i, j) stream.  Thread per (row, channel); a row's
// DH lanes run together (they leave together: the exits below depend on the row only).
__device__ __forceinline__ float keep_scale(const AttnArgs& a, uint32_t off, int i, int j) {
  if (a.thresh8) {
    const u32x4_t r = philox4x32_10((uint32_t)(i >> 2), (uint32_t)(16 * (j >> 6) + (j & 15)), off, a.c3, a.seed);
    return qbyte(r, (j >> 4) & 3, i & 3) >= a.thresh8 ? a.inv_keep : 0.f;
  }
  if (a.thresh) return keep_word(a.seed, off, a.c3, i, j) >= a.thresh ? a.inv_keep : 0.f;
  return 1.f;
}

template <int DH, bool GQA = false>
__global__ __launch_bounds__(256) void k_attn_dead_fwd(const AttnArgs a) {
  const int c = threadIdx.x % DH, i = blockIdx.x * (256 / DH) + threadIdx.x / DH;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H, n = a.n;
  const int len = a.lens[b];
  if (len <= 0 || i >= n || i < len + a.window) return;
  const int64_t ob = ebase(a, a.out, b) + h * a.out.sh;
  const int64_t ib = GQA ? ebase(a, a.kv, b) + kv_head_of(h, a.Hkv) * a.kv.sh : ebase(a, a.in, b) + h * a.in.sh;   // V
  const int isi = GQA ? a.kv.si : a.in.si;
  const uint32_t off = a.offset + (uint32_t)bh;
  // (the DH lanes of a row each draw the keep factor of one key and hand it round: one Philox
  // block per (row, key), not per channel)
  float acc = 0.f;
  for (int j0 = 0; j0 < n; j0 += DH) {
    const float zm = j0 + c < n ? keep_scale(a, off, i, j0 + c) : 0.f;
    for (int jj = 0; jj < DH; ++jj) {
      const float z = __shfl(zm, jj, DH);
      if (j0 + jj < n) acc += z * a.V[ib + (int64_t)(j0 + jj) * isi + c];
    }
  }
  const float ov = acc / (float)n;
  const int64_t at = ob + (int64_t)i * a.out.si + c;
  a.Oout[at] = ov;
  if (a.OGout) a.OGout[at] = ov * sigmoidf_(a.G[ebase(a, a.gate, b) + h * a.gate.sh + (int64_t)i * a.gate.si + c]);
}

// GQA: the grid is (rows, b Hkv) and the thread adds the parts of its kv head's query heads in ascending
// order before the one read-modify-write of dV (per query head, several would meet on one kv head's dV)
template <int DH, bool GQA = false>
__global__ __launch_bounds__(256) void k_attn_dead_bwd(const AttnArgs a) {
  const int c = threadIdx.x % DH, j = blockIdx.x * (256 / DH) + threadIdx.x / DH;
  const int nhk = GQA ? a.Hkv : a.H;
  const int b = blockIdx.y / nhk, hk = blockIdx.y - b * nhk, n = a.n;
  const int len = a.lens[b];
  if (len <= 0 || j >= n) return;
  const int64_t gb = GQA ? ebase(a, a.kvgrad, b) + hk * a.kvgrad.sh : ebase(a, a.grad, b) + hk * a.grad.sh;
  const int gsi = GQA ? a.kvgrad.si : a.grad.si;
  float acc = 0.f;
  for (int g = 0; g < (GQA ? a.H : 1); ++g) {
    const int h = GQA ? g : hk;
    if (GQA && kv_head_of(h, a.Hkv) != hk) continue;   // (uniform over the workgroup)
    const int64_t ob = ebase(a, a.out, b) + h * a.out.sh;
    const uint32_t off = a.offset + (uint32_t)(b * a.H + h);
    for (int i0 = len + a.window; i0 < n; i0 += DH) {
      const float zm = i0 + c < n ? keep_scale(a, off, i0 + c, j) : 0.f;
      for (int ii = 0; ii < DH; ++ii) {
        const float z = __shfl(zm, ii, DH);
        if (i0 + ii < n) acc += z * a.dO[ob + (int64_t)(i0 + ii) * a.out.si + c];
      }
    }
  }
  if (len + a.window < n) a.dV[gb + (int64_t)j * gsi + c] += acc / (float)n;
}

// ---------------------------------------------------------------------------------------------
// Sink backward (M > 0), after the backward of the real keys on the same stream.  One workgroup per
// (b, h) walks the head's rows in chunks of SB_ROWS, a thread per row:
//   P_im = exp(scale q_i . mem_k[g, m] - lse_i), dS_im = P_im (z_im dO_i . mem_v[g, m] - D_i) with D_i =
//   rowsum(dO_i * O_i) formed here (the order of k_attn_bwd_dkdv's sum), dq_i += scale sum_m dS_im mem_k[g, m]
// and leaves dS and P~ = z P of the chunk in LDS; then thread (m, c) adds the chunk's rows, ascending,
// into its elements of the head's partials  dmem_k[m][c] = scale sum_i dS_im q_i[c],  dmem_v[m][c] =
// sum_i P~_im dO_i[c].  The rows are all the step holds: n (padded layout) or min(len, n) (packed).
// k_attn_sink_reduce sums the partials over b and over a kv head's query heads in ascending order: no
// atomics, the same bits every run.  (The zero key has no gradient of its own: it is in lse.)
// CAP = true (a.cap > 0): P_im is that of the clamped score cap tanh(scale q_i . mem_k / cap) and the dS that
// feeds dq and dmem_k carries 1 - tanh^2; P~ (dmem_v) does not change
constexpr int SB_ROWS = 256, SB_ST = kMaxMemKV + 1;
template <int DH, bool CAP = false>
__global__ __launch_bounds__(256) void k_attn_sink_bwd(const AttnArgs a) {
  constexpr int EU = kMaxMemKV * DH / 256;   // (m, c) elements per thread
  __shared__ float mk[kMaxMemKV][DH], mv[kMaxMemKV][DH];
  __shared__ float dSs[SB_ROWS][SB_ST], Pds[SB_ROWS][SB_ST];
  const int tid = threadIdx.x;
  const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H, ns = a.n;
  const int len = a.lens[b];
  const int n = a.ep_off ? min(len, ns) : ns;   // packed rows: the episode's own length
  const int M = a.M;
  const int64_t ib = ebase(a, a.in, b) + h * a.in.sh, ob = ebase(a, a.out, b) + h * a.out.sh, gb = ebase(a, a.grad, b) + h * a.grad.sh;
  const int isi = a.in.si, osi = a.out.si, gsi = a.grad.si;
  const uint32_t off = a.offset + (uint32_t)bh;
  {
    const int64_t mb = (int64_t)kv_head_of(h, a.Hkv) * M * DH;
    for (int x = tid; x < M * DH; x += 256) {
      mk[x / DH][x % DH] = a.MK[mb + x];
      mv[x / DH][x % DH] = a.MV[mb + x];
    }
  }
  float ak[EU], av[EU];
#pragma unroll
  for (int u = 0; u < EU; ++u) ak[u] = av[u] = 0.f;
  for (int i0 = 0; i0 < n; i0 += SB_ROWS) {
    __syncthreads();   // mk / mv staged; the chunk before is summed
    const int i = i0 + tid;
    if (i < n) {
      float qr[DH], dor[DH], dq[DH];
      float dsum = 0.f;
#pragma unroll
      for (int c = 0; c < DH; ++c) {
        qr[c] = a.Q[ib + (int64_t)i * isi + c];
        dor[c] = a.dO[ob + (int64_t)i * osi + c];
        dq[c] = 0.f;
      }
#pragma unroll
      for (int c = 0; c < DH; ++c) dsum += dor[c] * a.O[ob + (int64_t)i * osi + c];
      const float lse = a.LSE[(int64_t)bh * ns + i];
      for (int m = 0; m < M; ++m) {
        float t = 0.f, gd = 0.f;
#pragma unroll
        for (int c = 0; c < DH; ++c) {
          t += qr[c] * mk[m][c];
          gd += dor[c] * mv[m][c];
        }
        float sc = t * a.scale, dt = 1.f;
        if constexpr (CAP) {
          const float th = tanhf(sc * a.inv_cap);
          sc = a.cap * th;
          dt = 1.f - th * th;
        }
        const float p = expf(sc - lse);
        float z = 1.f;
        if (a.thresh) z = keep_word(a.seed, off, a.c3, i, (int)(SINK_C1 | (uint32_t)m)) >= a.thresh ? a.inv_keep : 0.f;
        const float ds = CAP ? p * (gd * z - dsum) * dt : p * (gd * z - dsum);
        dSs[tid][m] = ds;
        Pds[tid][m] = p * z;
#pragma unroll
        for (int c = 0; c < DH; ++c) dq[c] += ds * mk[m][c];
      }
#pragma unroll
      for (int c = 0; c < DH; ++c) a.dQ[gb + (int64_t)i * gsi + c] += dq[c] * a.scale;
    }
    __syncthreads();
    const int rows = min(SB_ROWS, n - i0);
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int e = tid + 256 * u, m = e / DH, c = e - m * DH;
      if (m < M) {
        for (int ii = 0; ii < rows; ++ii) {
          ak[u] += dSs[ii][m] * a.Q[ib + (int64_t)(i0 + ii) * isi + c];
          av[u] += Pds[ii][m] * a.dO[ob + (int64_t)(i0 + ii) * osi + c];
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < EU; ++u) {
    const int e = tid + 256 * u;
    if (e < M * DH) {
      a.dMKp[(int64_t)bh * M * DH + e] = ak[u] * a.scale;
      a.dMVp[(int64_t)bh * M * DH + e] = av[u];
    }
  }
}

// dmem_k / dmem_v [Hkv][M][dh] = (dm_accum: +=) the partials summed over b, then over the kv head's query
// heads, both ascending; thread per element
__global__ __launch_bounds__(256) void k_attn_sink_reduce(const AttnArgs a, int B, int dh) {
  const int x = blockIdx.x * 256 + threadIdx.x, per = a.M * dh;
  if (x >= a.Hkv * per) return;
  const int g = x / per, e = x - g * per;
  float sk = 0.f, sv = 0.f;
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < a.H; ++h) {
      if (kv_head_of(h, a.Hkv) != g) continue;
      sk += a.dMKp[(int64_t)(b * a.H + h) * per + e];
      sv += a.dMVp[(int64_t)(b * a.H + h) * per + e];
    }
  a.dMK[x] = a.dm_accum ? a.dMK[x] + sk : sk;
  a.dMV[x] = a.dm_accum ? a.dMV[x] + sv : sv;
}

// whether a problem can have such rows: a window, the padded layout, and a row n - 1 >= 1 + W — and no
// sink (with one, a row without a visible key attends the sinks alone)
bool has_dead_rows(const AttnProblem& p) {
  return p.window > 0 && !p.ep_off && p.window <= p.n - 2 && !attn_has_sinks(p);
}

// grouped-query attention proper: fewer kv heads than query heads (Hkv = 0 or H: today's kernels)
bool is_gqa(const AttnProblem& p) { return p.Hkv > 0 && p.Hkv < p.H; }

bool attn_fused_bwd_on() {   // XTRL_ATTN_FUSED_BWD=0: the kernel pair (read per launch: tests flip it)
  const char* e = getenv("XTRL_ATTN_FUSED_BWD");
  return !(e && atoi(e) == 0);
}

int fill_args(AttnArgs& a, const AttnProblem& p) {
  XTRL_REQUIRE(p.dh == 16 || p.dh == 32 || p.dh == 64, "attn: dim_head %d unsupported (16/32/64)", p.dh);
  XTRL_REQUIRE(p.lens && p.H > 0 && p.n > 0 && p.b > 0, "attn: bad arguments");
  XTRL_REQUIRE(p.dropout >= 0.f && p.dropout < 1.f, "attn: dropout %f outside [0, 1)", p.dropout);
  a.lens = p.lens;
  a.H = p.H;
  a.n = p.n;
  a.in = p.in;
  a.out = p.out;
  a.grad = p.grad;
  a.gate = p.gate;
  a.scale = p.scale;
  a.inv_keep = p.dropout > 0.f ? 1.f / (1.f - p.dropout) : 1.f;
  a.thresh = dropout_thresh(p.dropout);
  a.thresh8 = dropout_thresh8(p.dropout);
  a.seed = p.seed;
  a.offset = p.offset;
  XTRL_REQUIRE(p.sub < (1u << 23), "attn: dropout stream sub-index %u does not fit 23 bits", p.sub);
  a.c3 = rng_c3(FIELD_DROPOUT, a.thresh8 ? (p.sub | (1u << 23)) : p.sub);
  a.causal = p.causal;
  a.ep_off = p.ep_off;
  XTRL_REQUIRE(p.window >= 0, "attn: window %d < 0 (0 = no window)", p.window);
  XTRL_REQUIRE(p.window == 0 || p.causal, "attn: a window needs causal attention");
  a.window = p.window > 0 ? min(p.window, NO_WINDOW) : NO_WINDOW;
  XTRL_REQUIRE(p.Hkv >= 0 && p.Hkv <= p.H && (p.Hkv == 0 || p.H % p.Hkv == 0),
               "attn: kv heads %d must divide heads %d (0 = heads)", p.Hkv, p.H);
  const bool gqa = is_gqa(p);
  a.Hkv = gqa ? p.Hkv : p.H;
  a.kv = gqa ? p.kv : p.in;
  a.kvgrad = gqa ? p.kvgrad : p.grad;
  XTRL_REQUIRE(p.mem_kv >= 0 && p.mem_kv <= kMaxMemKV, "attn: num_mem_kv %d outside [0, %d]", p.mem_kv, kMaxMemKV);
  XTRL_REQUIRE(p.mem_kv == 0 || (p.mem_k && p.mem_v), "attn: num_mem_kv %d without mem_k / mem_v", p.mem_kv);
  XTRL_REQUIRE(!attn_has_sinks(p) || p.causal, "attn: the sinks need causal attention");
  a.MK = p.mem_k;
  a.MV = p.mem_v;
  a.M = p.mem_kv;
  a.Z = p.zero_kv ? 1 : 0;
  XTRL_REQUIRE(!p.alibi || p.causal, "attn: ALiBi needs causal attention");
  a.alibi = p.alibi;   // (its forms are the GQA ones: a.Hkv = H, a.kv = in, a.kvgrad = grad above serve Hkv = H)
  XTRL_REQUIRE(p.softclamp >= 0.f && std::isfinite(p.softclamp),
               "attn: softclamp %g is negative or not finite (0 = off)", (double)p.softclamp);
  XTRL_REQUIRE(p.softclamp == 0.f || p.causal, "attn: the logit soft-clamp needs causal attention");
  a.cap = p.softclamp;   // (its forms are the ALiBi ones, a.alibi NULL included)
  a.inv_cap = p.softclamp > 0.f ? 1.f / p.softclamp : 0.f;
  return XTRL_OK;
}

// the sink part of the backward (M > 0), after the real keys' kernels: dQ += ..., dmem_k / dmem_v
int sink_bwd(AttnArgs& a, const AttnProblem& p, hipStream_t s) {
  if (p.mem_kv <= 0) return XTRL_OK;
  XTRL_REQUIRE(p.dmem_k && p.dmem_v, "attn_bwd: num_mem_kv %d without dmem_k / dmem_v", p.mem_kv);
  const int64_t need = attn_sink_ws_floats(p.b, p.H, p.mem_kv, p.dh);
  XTRL_REQUIRE(p.sink_ws && p.sink_ws_floats >= need, "attn_bwd: sink workspace %lld < %lld floats",
               (long long)p.sink_ws_floats, (long long)need);
  a.dMKp = p.sink_ws;
  a.dMVp = p.sink_ws + need / 2;
  a.dMK = p.dmem_k;
  a.dMV = p.dmem_v;
  a.dm_accum = p.dmem_accum;
  if (p.softclamp > 0.f) XTRL_LAUNCH_DH(p.dh, k_attn_sink_bwd, (true), dim3(p.b * p.H), dim3(256), 0, s, a);
  else XTRL_LAUNCH_DH(p.dh, k_attn_sink_bwd, (false), dim3(p.b * p.H), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_attn_sink_reduce, dim3((a.Hkv * p.mem_kv * p.dh + 255) / 256), dim3(256), 0, s, a, p.b, p.dh);
  XTRL_LAUNCHED("attn_sink_bwd");
  return XTRL_OK;
}

// the sum of the per-key-tile dQ partials that k_attn_bwd_dkdv<16, true, ...> left in a.dQp
void dq_reduce(const AttnArgs& a, const AttnProblem& p, hipStream_t s) {
  const int64_t units = (int64_t)p.b * p.H * p.n * 4;
  hipLaunchKernelGGL(k_attn_dq_reduce<16>, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, a, p.b * p.H);
}

// The general forms of the backward — GQA, on it ALiBi, on that the soft-clamp — take the kv head mapping
// and the window at run time.  The dK / dV grid is over the kv heads (the group loop; a.Hkv = H without
// grouped-query attention: a group of one query head per kv head), the dQ side stays per query head.  The
// one-launch fused backward has no group loop: `part` (dh = 16, the caller gave the dQ partial workspace)
// takes the dK / dV kernel with the dQ pass folded in, else the kernel pair
template <bool ALIBI, bool CAP>
void bwd_general(AttnArgs& a, const AttnProblem& p, bool part, dim3 grid, hipStream_t s) {
  dim3 kgrid((p.n + TK - 1) / TK, p.b * a.Hkv);
  if (part) {
    a.dQp = p.dq_part;
    hipLaunchKernelGGL((k_attn_bwd_dkdv<16, true, true, true, ALIBI, CAP>), kgrid, dim3(256), 0, s, a);
    dq_reduce(a, p, s);
  } else {
    XTRL_LAUNCH_DH(p.dh, k_attn_bwd_dkdv, (false, true, true, ALIBI, CAP), kgrid, dim3(256), 0, s, a);
    XTRL_LAUNCH_DH(p.dh, k_attn_bwd_dq, (true, ALIBI, CAP), grid, dim3(256), 0, s, a);
  }
}

}  // namespace

int attn_fwd_ex(const AttnProblem& p, const float* q, const float* k, const float* v, float* o, float* lse,
                const float* gate, float* og, hipStream_t s) {
  AttnArgs a{};
  if (int rc = fill_args(a, p)) return rc;
  XTRL_REQUIRE(q && k && v && o && lse, "attn_fwd: null operand");
  XTRL_REQUIRE(!gate == !og, "attn_fwd: gate and og go together");
  a.Q = q;
  a.K = k;
  a.V = v;
  a.Oout = o;
  a.LSEout = lse;
  a.G = gate;
  a.OGout = og;
  const bool gqa = is_gqa(p);
  dim3 grid((p.n + TQ - 1) / TQ, p.b * p.H);
  const bool sinks = attn_has_sinks(p);
  // k_attn_fwd<DH, GQA, SINK, ALIBI, CAP>: every form from the sink one up takes the kv head mapping at run
  // time (Hkv = H included); the ALiBi and soft-clamp forms come with and without sinks, the soft-clamp
  // ones with slopes or none
  switch (attn_form(p.softclamp > 0.f, p.alibi != nullptr, sinks, gqa)) {
    case ATTN_CLAMP:
      if (sinks) XTRL_LAUNCH_DH(p.dh, k_attn_fwd, (true, true, true, true), grid, dim3(256), 0, s, a);
      else XTRL_LAUNCH_DH(p.dh, k_attn_fwd, (true, false, true, true), grid, dim3(256), 0, s, a);
      break;
    case ATTN_ALIBI:
      if (sinks) XTRL_LAUNCH_DH(p.dh, k_attn_fwd, (true, true, true), grid, dim3(256), 0, s, a);
      else XTRL_LAUNCH_DH(p.dh, k_attn_fwd, (true, false, true), grid, dim3(256), 0, s, a);
      break;
    case ATTN_SINK: XTRL_LAUNCH_DH(p.dh, k_attn_fwd, (true, true), grid, dim3(256), 0, s, a); break;
    case ATTN_GQA: XTRL_LAUNCH_DH(p.dh, k_attn_fwd, (true), grid, dim3(256), 0, s, a); break;
    case ATTN_PLAIN: XTRL_LAUNCH_DH(p.dh, k_attn_fwd, (false), grid, dim3(256), 0, s, a); break;
  }
  XTRL_LAUNCHED("attn_fwd");
  if (has_dead_rows(p)) {
    dim3 dgrid((p.n + 256 / p.dh - 1) / (256 / p.dh), p.b * p.H);
    if (gqa) XTRL_LAUNCH_DH(p.dh, k_attn_dead_fwd, (true), dgrid, dim3(256), 0, s, a);
    else XTRL_LAUNCH_DH(p.dh, k_attn_dead_fwd, (false), dgrid, dim3(256), 0, s, a);
    XTRL_LAUNCHED("attn_dead_fwd");
  }
  return XTRL_OK;
}

int attn_bwd_ex(const AttnProblem& p, const float* q, const float* k, const float* v, const float* o,
                const float* lse, const float* dout, float* dq, float* dk, float* dv, float* delta_ws,
                hipStream_t s) {
  AttnArgs a{};
  if (int rc = fill_args(a, p)) return rc;
  XTRL_REQUIRE(q && k && v && o && lse && dout && dq && dk && dv && delta_ws, "attn_bwd: null operand");
  XTRL_REQUIRE(p.causal, "attn_bwd: bidirectional attention is forward-only");
  a.Q = q;
  a.K = k;
  a.V = v;
  a.O = o;
  a.LSE = lse;
  a.dO = dout;
  a.Dl = delta_ws;
  a.Dout = delta_ws;
  a.dQ = dq;
  a.dK = dk;
  a.dV = dv;
  // (D = rowsum(dO * O) is formed inside k_attn_bwd_dkdv, whose diagonal workgroups store it for dq)
  dim3 grid((p.n + TQ - 1) / TQ, p.b * p.H);
  const int64_t part_need = attn_dq_part_floats(p.b, p.H, p.n, p.dh);
  const bool gqa = is_gqa(p);
  // XTRL_ATTN_FUSED_BWD=0 turns off both forms with the dQ pass folded in, the one launch and the partials
  const bool fused_on = p.dh == 16 && attn_fused_bwd_on();
  const bool part = fused_on && p.dq_part && p.dq_part_floats >= part_need;
  // the sinks choose no form here: lse and o carry their share into the real keys' kernels, sink_bwd adds theirs
  switch (attn_form(p.softclamp > 0.f, p.alibi != nullptr, false, gqa)) {
    case ATTN_CLAMP: bwd_general<true, true>(a, p, part, grid, s); break;   // slopes or none
    case ATTN_ALIBI: bwd_general<true, false>(a, p, part, grid, s); break;
    case ATTN_GQA: bwd_general<false, false>(a, p, part, grid, s); break;
    default:   // one kv head per query head, no option: the window is a template flag at dh = 16
      if (fused_on && p.n <= FB_MAXN) {   // short episodes: one fused launch
        hipLaunchKernelGGL(k_attn_bwd_fused<16>, dim3(p.b * p.H), dim3(256), 0, s, a);
      } else if (part) {
        // long episodes: dK / dV with the dQ pass folded in (partials for multi-key-tile rows) + their sum
        a.dQp = p.dq_part;
        if (p.window > 0) hipLaunchKernelGGL((k_attn_bwd_dkdv<16, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_attn_bwd_dkdv<16, true, false>), grid, dim3(256), 0, s, a);
        dq_reduce(a, p, s);
      } else {
        if (p.dh == 16 && p.window <= 0) hipLaunchKernelGGL((k_attn_bwd_dkdv<16, false, false>), grid, dim3(256), 0, s, a);
        else XTRL_LAUNCH_DH(p.dh, k_attn_bwd_dkdv, (false, true), grid, dim3(256), 0, s, a);
        XTRL_LAUNCH_DH(p.dh, k_attn_bwd_dq, (false), grid, dim3(256), 0, s, a);
      }
  }
  XTRL_LAUNCHED("attn_bwd");
  if (has_dead_rows(p)) {
    dim3 dgrid((p.n + 256 / p.dh - 1) / (256 / p.dh), p.b * a.Hkv);
    if (gqa) XTRL_LAUNCH_DH(p.dh, k_attn_dead_bwd, (true), dgrid, dim3(256), 0, s, a);
    else XTRL_LAUNCH_DH(p.dh, k_attn_dead_bwd, (false), dgrid, dim3(256), 0, s, a);
    XTRL_LAUNCHED("attn_dead_bwd");
  }
  return sink_bwd(a, p, s);
}

int64_t attn_dq_part_floats(int b, int H, int n, int dh) {
  return (int64_t)((n + TK - 1) / TK) * b * H * n * dh;
}

// per-(b, h) partials of dmem_k and of dmem_v
int64_t attn_sink_ws_floats(int b, int H, int mem_kv, int dh) { return 2 * (int64_t)b * H * mem_kv * dh; }

AttnProblem contiguous_problem(const int32_t* lens, int b, int H, int n, int dh, float scale, float p, uint64_t seed,
                               uint32_t offset, uint32_t sub, int window, int Hkv) {
  AttnProblem pr{b, H, n, dh, lens, scale, p, seed, offset, {}, {}, {}, {}};
  pr.sub = sub;
  pr.window = window;
  pr.in = pr.out = pr.grad = attn_layout_bhnd(H, n, dh);
  pr.Hkv = Hkv;   // k, v, dk, dv [b][Hkv][n][dh] (checked by fill_args)
  if (Hkv > 0) pr.kv = pr.kvgrad = attn_layout_bhnd(Hkv, n, dh);
  return pr;
}

}  // namespace xtrl

extern "C" int xtrl_attn_fwd_softclamp(const float* q, const float* k, const float* v, const int32_t* lens, float* o,
                                       float* lse, const float* mem_k, const float* mem_v, int b, int H, int Hkv,
                                       int n, int dh, float scale, float dropout_p, uint64_t seed, uint32_t offset,
                                       uint32_t sub, int window, int num_mem_kv, int add_zero_kv,
                                       const float* alibi_slopes, float softclamp, void* stream) {
  XTRL_REQUIRE(Hkv >= 1, "attn_fwd: kv heads %d < 1", Hkv);
  xtrl::AttnProblem pr = xtrl::contiguous_problem(lens, b, H, n, dh, scale, dropout_p, seed, offset, sub, window, Hkv);
  pr.mem_k = mem_k;
  pr.mem_v = mem_v;
  pr.mem_kv = num_mem_kv;
  pr.zero_kv = add_zero_kv;
  pr.alibi = alibi_slopes;
  pr.softclamp = softclamp;
  return xtrl::attn_fwd_ex(pr, q, k, v, o, lse, nullptr, nullptr, xtrl::as_stream(stream));
}

extern "C" int xtrl_attn_fwd_alibi(const float* q, const float* k, const float* v, const int32_t* lens, float* o,
                                   float* lse, const float* mem_k, const float* mem_v, int b, int H, int Hkv, int n,
                                   int dh, float scale, float dropout_p, uint64_t seed, uint32_t offset, uint32_t sub,
                                   int window, int num_mem_kv, int add_zero_kv, const float* alibi_slopes,
                                   void* stream) {
  return xtrl_attn_fwd_softclamp(q, k, v, lens, o, lse, mem_k, mem_v, b, H, Hkv, n, dh, scale, dropout_p, seed, offset,
                                 sub, window, num_mem_kv, add_zero_kv, alibi_slopes, 0.f, stream);
}

extern "C" int xtrl_attn_fwd_sink(const float* q, const float* k, const float* v, const int32_t* lens, float* o,
                                  float* lse, const float* mem_k, const float* mem_v, int b, int H, int Hkv, int n,
                                  int dh, float scale, float dropout_p, uint64_t seed, uint32_t offset, uint32_t sub,
                                  int window, int num_mem_kv, int add_zero_kv, void* stream) {
  return xtrl_attn_fwd_alibi(q, k, v, lens, o, lse, mem_k, mem_v, b, H, Hkv, n, dh, scale, dropout_p, seed, offset, sub,
                             window, num_mem_kv, add_zero_kv, nullptr, stream);
}

extern "C" int xtrl_attn_fwd_gqa(const float* q, const float* k, const float* v, const int32_t* lens, float* o,
                                 float* lse, int b, int H, int Hkv, int n, int dh, float scale, float dropout_p,
                                 uint64_t seed, uint32_t offset, uint32_t sub, int window, void* stream) {
  return xtrl_attn_fwd_sink(q, k, v, lens, o, lse, nullptr, nullptr, b, H, Hkv, n, dh, scale, dropout_p, seed, offset,
                            sub, window, 0, 0, stream);
}

extern "C" int xtrl_attn_fwd_win(const float* q, const float* k, const float* v, const int32_t* lens, float* o,
                                 float* lse, int b, int H, int n, int dh, float scale, float dropout_p, uint64_t seed,
                                 uint32_t offset, uint32_t sub, int window, void* stream) {
  return xtrl_attn_fwd_gqa(q, k, v, lens, o, lse, b, H, H, n, dh, scale, dropout_p, seed, offset, sub, window, stream);
}

extern "C" int xtrl_attn_fwd(const float* q, const float* k, const float* v, const int32_t* lens, float* o,
                             float* lse, int b, int H, int n, int dh, float scale, float dropout_p, uint64_t seed,
                             uint32_t offset, uint32_t sub, void* stream) {
  return xtrl_attn_fwd_win(q, k, v, lens, o, lse, b, H, n, dh, scale, dropout_p, seed, offset, sub, 0, stream);
}

extern "C" int64_t xtrl_attn_bwd_part_floats(int b, int H, int n, int dh) {
  return xtrl::attn_dq_part_floats(b, H, n, dh);
}

extern "C" int64_t xtrl_attn_sink_ws_floats(int b, int H, int num_mem_kv, int dh) {
  return xtrl::attn_sink_ws_floats(b, H, num_mem_kv, dh);
}

extern "C" int xtrl_attn_bwd_part_softclamp(const float* q, const float* k, const float* v, const int32_t* lens,
                                            const float* o, const float* lse, const float* dout, float* dq, float* dk,
                                            float* dv, float* delta_ws, float* dq_part, int64_t dq_part_floats,
                                            const float* mem_k, const float* mem_v, float* dmem_k, float* dmem_v,
                                            float* sink_ws, int64_t sink_ws_floats, int b, int H, int Hkv, int n,
                                            int dh, float scale, float dropout_p, uint64_t seed, uint32_t offset,
                                            uint32_t sub, int window, int num_mem_kv, int add_zero_kv,
                                            const float* alibi_slopes, float softclamp, void* stream) {
  XTRL_REQUIRE(Hkv >= 1, "attn_bwd: kv heads %d < 1", Hkv);
  xtrl::AttnProblem pr = xtrl::contiguous_problem(lens, b, H, n, dh, scale, dropout_p, seed, offset, sub, window, Hkv);
  pr.dq_part = dq_part;
  pr.dq_part_floats = dq_part_floats;
  pr.mem_k = mem_k;
  pr.mem_v = mem_v;
  pr.mem_kv = num_mem_kv;
  pr.zero_kv = add_zero_kv;
  pr.dmem_k = dmem_k;
  pr.dmem_v = dmem_v;
  pr.sink_ws = sink_ws;
  pr.sink_ws_floats = sink_ws_floats;
  pr.alibi = alibi_slopes;
  pr.softclamp = softclamp;
  return xtrl::attn_bwd_ex(pr, q, k, v, o, lse, dout, dq, dk, dv, delta_ws, xtrl::as_stream(stream));
}

extern "C" int xtrl_attn_bwd_softclamp(const float* q, const float* k, const float* v, const int32_t* lens,
                                       const float* o, const float* lse, const float* dout, float* dq, float* dk,
                                       float* dv, float* delta_ws, const float* mem_k, const float* mem_v,
                                       float* dmem_k, float* dmem_v, float* sink_ws, int64_t sink_ws_floats, int b,
                                       int H, int Hkv, int n, int dh, float scale, float dropout_p, uint64_t seed,
                                       uint32_t offset, uint32_t sub, int window, int num_mem_kv, int add_zero_kv,
                                       const float* alibi_slopes, float softclamp, void* stream) {
  return xtrl_attn_bwd_part_softclamp(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, nullptr, 0, mem_k, mem_v,
                                      dmem_k, dmem_v, sink_ws, sink_ws_floats, b, H, Hkv, n, dh, scale, dropout_p, seed,
                                      offset, sub, window, num_mem_kv, add_zero_kv, alibi_slopes, softclamp, stream);
}

extern "C" int xtrl_attn_bwd_part_alibi(const float* q, const float* k, const float* v, const int32_t* lens,
                                        const float* o, const float* lse, const float* dout, float* dq, float* dk,
                                        float* dv, float* delta_ws, float* dq_part, int64_t dq_part_floats,
                                        const float* mem_k, const float* mem_v, float* dmem_k, float* dmem_v,
                                        float* sink_ws, int64_t sink_ws_floats, int b, int H, int Hkv, int n, int dh,
                                        float scale, float dropout_p, uint64_t seed, uint32_t offset, uint32_t sub,
                                        int window, int num_mem_kv, int add_zero_kv, const float* alibi_slopes,
                                        void* stream) {
  return xtrl_attn_bwd_part_softclamp(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, dq_part, dq_part_floats, mem_k,
                                      mem_v, dmem_k, dmem_v, sink_ws, sink_ws_floats, b, H, Hkv, n, dh, scale,
                                      dropout_p, seed, offset, sub, window, num_mem_kv, add_zero_kv, alibi_slopes, 0.f,
                                      stream);
}

extern "C" int xtrl_attn_bwd_alibi(const float* q, const float* k, const float* v, const int32_t* lens, const float* o,
                                   const float* lse, const float* dout, float* dq, float* dk, float* dv, float* delta_ws,
                                   const float* mem_k, const float* mem_v, float* dmem_k, float* dmem_v, float* sink_ws,
                                   int64_t sink_ws_floats, int b, int H, int Hkv, int n, int dh, float scale,
                                   float dropout_p, uint64_t seed, uint32_t offset, uint32_t sub, int window,
                                   int num_mem_kv, int add_zero_kv, const float* alibi_slopes, void* stream) {
  return xtrl_attn_bwd_part_alibi(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, nullptr, 0, mem_k, mem_v, dmem_k,
                                  dmem_v, sink_ws, sink_ws_floats, b, H, Hkv, n, dh, scale, dropout_p, seed, offset,
                                  sub, window, num_mem_kv, add_zero_kv, alibi_slopes, stream);
}

extern "C" int xtrl_attn_bwd_part_sink(const float* q, const float* k, const float* v, const int32_t* lens,
                                       const float* o, const float* lse, const float* dout, float* dq, float* dk,
                                       float* dv, float* delta_ws, float* dq_part, int64_t dq_part_floats,
                                       const float* mem_k, const float* mem_v, float* dmem_k, float* dmem_v,
                                       float* sink_ws, int64_t sink_ws_floats, int b, int H, int Hkv, int n, int dh,
                                       float scale, float dropout_p, uint64_t seed, uint32_t offset, uint32_t sub,
                                       int window, int num_mem_kv, int add_zero_kv, void* stream) {
  return xtrl_attn_bwd_part_alibi(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, dq_part, dq_part_floats, mem_k,
                                  mem_v, dmem_k, dmem_v, sink_ws, sink_ws_floats, b, H, Hkv, n, dh, scale, dropout_p,
                                  seed, offset, sub, window, num_mem_kv, add_zero_kv, nullptr, stream);
}

extern "C" int xtrl_attn_bwd_sink(const float* q, const float* k, const float* v, const int32_t* lens, const float* o,
                                  const float* lse, const float* dout, float* dq, float* dk, float* dv, float* delta_ws,
                                  const float* mem_k, const float* mem_v, float* dmem_k, float* dmem_v, float* sink_ws,
                                  int64_t sink_ws_floats, int b, int H, int Hkv, int n, int dh, float scale,
                                  float dropout_p, uint64_t seed, uint32_t offset, uint32_t sub, int window,
                                  int num_mem_kv, int add_zero_kv, void* stream) {
  return xtrl_attn_bwd_part_sink(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, nullptr, 0, mem_k, mem_v, dmem_k,
                                 dmem_v, sink_ws, sink_ws_floats, b, H, Hkv, n, dh, scale, dropout_p, seed, offset, sub,
                                 window, num_mem_kv, add_zero_kv, stream);
}

extern "C" int xtrl_attn_bwd_part_gqa(const float* q, const float* k, const float* v, const int32_t* lens,
                                      const float* o, const float* lse, const float* dout, float* dq, float* dk,
                                      float* dv, float* delta_ws, float* dq_part, int64_t dq_part_floats, int b, int H,
                                      int Hkv, int n, int dh, float scale, float dropout_p, uint64_t seed,
                                      uint32_t offset, uint32_t sub, int window, void* stream) {
  return xtrl_attn_bwd_part_sink(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, dq_part, dq_part_floats, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, 0, b, H, Hkv, n, dh, scale, dropout_p, seed,
                                 offset, sub, window, 0, 0, stream);
}

extern "C" int xtrl_attn_bwd_part_win(const float* q, const float* k, const float* v, const int32_t* lens,
                                      const float* o, const float* lse, const float* dout, float* dq, float* dk,
                                      float* dv, float* delta_ws, float* dq_part, int64_t dq_part_floats, int b, int H,
                                      int n, int dh, float scale, float dropout_p, uint64_t seed, uint32_t offset,
                                      uint32_t sub, int window, void* stream) {
  return xtrl_attn_bwd_part_gqa(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, dq_part, dq_part_floats, b, H, H, n,
                                dh, scale, dropout_p, seed, offset, sub, window, stream);
}

extern "C" int xtrl_attn_bwd_part(const float* q, const float* k, const float* v, const int32_t* lens, const float* o,
                                  const float* lse, const float* dout, float* dq, float* dk, float* dv, float* delta_ws,
                                  float* dq_part, int64_t dq_part_floats, int b, int H, int n, int dh, float scale,
                                  float dropout_p, uint64_t seed, uint32_t offset, uint32_t sub, void* stream) {
  return xtrl_attn_bwd_part_win(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, dq_part, dq_part_floats, b, H, n, dh,
                                scale, dropout_p, seed, offset, sub, 0, stream);
}

extern "C" int xtrl_attn_bwd_gqa(const float* q, const float* k, const float* v, const int32_t* lens, const float* o,
                                 const float* lse, const float* dout, float* dq, float* dk, float* dv, float* delta_ws,
                                 int b, int H, int Hkv, int n, int dh, float scale, float dropout_p, uint64_t seed,
                                 uint32_t offset, uint32_t sub, int window, void* stream) {
  return xtrl_attn_bwd_sink(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, nullptr, nullptr, nullptr, nullptr,
                            nullptr, 0, b, H, Hkv, n, dh, scale, dropout_p, seed, offset, sub, window, 0, 0, stream);
}

extern "C" int xtrl_attn_bwd_win(const float* q, const float* k, const float* v, const int32_t* lens, const float* o,
                                 const float* lse, const float* dout, float* dq, float* dk, float* dv, float* delta_ws,
                                 int b, int H, int n, int dh, float scale, float dropout_p, uint64_t seed,
                                 uint32_t offset, uint32_t sub, int window, void* stream) {
  return xtrl_attn_bwd_gqa(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, b, H, H, n, dh, scale, dropout_p, seed,
                           offset, sub, window, stream);
}

extern "C" int xtrl_attn_bwd(const float* q, const float* k, const float* v, const int32_t* lens, const float* o,
                             const float* lse, const float* dout, float* dq, float* dk, float* dv, float* delta_ws,
                             int b, int H, int n, int dh, float scale, float dropout_p, uint64_t seed,
                             uint32_t offset, uint32_t sub, void* stream) {
  return xtrl_attn_bwd_win(q, k, v, lens, o, lse, dout, dq, dk, dv, delta_ws, b, H, n, dh, scale, dropout_p, seed,
                           offset, sub, 0, stream);
}

/* bidirectional / causal attention forward on token-major operands (rows b * n + i, head h at
 * columns h * dh): q, k, v with row strides ldq / ldk / ldv, out o [b * n][ldo].
 * Precondition: lens[b] >= 1 (no window here, so an episode without a valid key divides 0 by 0). */
extern "C" int xtrl_attn_fwd_tokens(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                    const int32_t* lens, float* o, int ldo, float* lse, int b, int H, int n, int dh,
                                    float scale, int causal, void* stream) {
  XTRL_REQUIRE(ldq == ldk && ldk == ldv, "attn_fwd_tokens: q, k, v share one row stride (got %d %d %d)", ldq, ldk,
               ldv);
  xtrl::AttnProblem pr{b, H, n, dh, lens, scale, 0.f, 0, 0, {}, {}, {}, {}};
  pr.in = xtrl::attn_layout_tokens(n, ldq, dh);
  pr.out = xtrl::attn_layout_tokens(n, ldo, dh);
  pr.causal = causal;
  // q, k, v are addressed from their own bases with the same layout
  return xtrl::attn_fwd_ex(pr, q, k, v, o, lse, nullptr, nullptr, (hipStream_t)stream);
}
