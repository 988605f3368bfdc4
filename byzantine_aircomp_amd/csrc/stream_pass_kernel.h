// The fused streaming Weiszfeld pass kernel (see stream_pass.hip for the algorithm): the
// template shared by the fp32 instantiations (stream_pass.hip) and the bf16-input ones
// (stream_pass_bf16.hip).
#pragma once
#include "device_util.h"
#include "gmagg_internal.h"
#include "philox.h"

// (waves per block, lanes per row segment, rows per thread, blocks per CU) fp32 tiles built
// (stream_pass.hip; stream_pass_cclip.hip builds the same set with SELF).
#define GMK_FOR_EACH_CFG(X_, V_)                                                             \
  X_(V_, 16, 64, 1, 1) X_(V_, 16, 64, 2, 1) X_(V_, 16, 64, 4, 1) X_(V_, 16, 64, 8, 1)        \
  X_(V_, 16, 32, 8, 1) X_(V_, 16, 16, 8, 1) X_(V_, 16, 8, 8, 1) X_(V_, 16, 4, 8, 1)          \
  X_(V_, 16, 4, 4, 1) X_(V_, 16, 16, 4, 1) X_(V_, 8, 8, 16, 1) X_(V_, 8, 4, 8, 1)            \
  X_(V_, 8, 16, 8, 1) X_(V_, 8, 8, 8, 1) X_(V_, 4, 8, 8, 1) X_(V_, 4, 16, 4, 1)              \
  X_(V_, 8, 32, 4, 1) X_(V_, 16, 8, 8, 2) X_(V_, 16, 16, 16, 1) X_(V_, 8, 8, 16, 2)          \
  X_(V_, 8, 32, 4, 4)                                                                        \
  X_(V_, 16, 32, 8, 2) X_(V_, 16, 64, 4, 2) X_(V_, 16, 64, 16, 1) X_(V_, 8, 16, 8, 2)

namespace gmk {

// B16: X holds bf16 elements.  The tile stays packed, two adjacent columns per VGPR (the
// low half is the even column), and an element is widened where it is used (xpair): exact,
// bf16 -> fp32 is `bits << 16`.  Expanded to fp32 the tile would take twice the registers
// and lose the occupancy the K <= 1024 tile's rate depends on.
// GB: the tile also carries the base iterate G at the finisher thread's column (the
// correction pass, DELTA = 2).  A base class, so that every other tile is the struct it was.
template <bool GB> struct TileBase {};
template <> struct TileBase<true> { float gb; };
template <int V, int R, bool B16 = false, bool GB = false>
struct Tile : TileBase<GB> {
  static_assert(!B16 || V == 8, "bf16 tiles: 8 columns = one 16-byte load per lane");
  typedef typename std::conditional<B16, uint32_t, float>::type word;
  word x[R][B16 ? V / 2 : V];
  float gold;    // finisher thread: g_t at its column (INIT: the guess)
  float hn;      // STEP finisher thread, host noise: its column's draw
};

// MODE: 0 step, 1 init, 2 init + ||x_k||^2, 3 Gram closing sum, 4 init after the OMA
// pre-noise (the tile gets the reference's per-client AWGN, M:385-394, in registers and is
// written back: one read + one write of X instead of OMA's read + write and INIT's read).  SCHED 0: load a
// chunk, then reduce it; 1 (PIPE): chunk c+1's loads are in flight while chunk
// c is reduced (two tiles of registers); 2 (ROLL): row i of chunk c+1 is loaded
// into the registers phase B has just freed (one tile).
// OCC: blocks per CU the register budget is capped for (2 -> <= 64 VGPRs at
// 16 waves); with OCC > 1 the row weights are read from LDS instead of VGPRs.
// PANEL: X is the panel layout [nch][K][J] (a.panel_stride elements between
// panels, rows J apart): a chunk is one contiguous block, every row offset in
// it fits the 32-bit lane offset, and the HBM stream is sequential.
// B16: bf16 elements (a.X is read as uint16_t; ldx / panel_stride count elements), V = 8;
// modes 0-2 only (mode 4 would round the noised values back to bf16: another algorithm).
// SELF (STEP only): the column term is the old iterate, g' = sum_k c_k x_k + a_noise * g_old
// (centered clipping; a.noise is 3 and no draw is added), with phase A's sums in fp64 (see
// there).  A template parameter, not a fourth runtime kind: gm2 / gm are to run the code
// they ran before.
// DELTA (gm2 STEP on panels, from the second STEP on): the two kernels of an
// iteration whose kind the K-space step has chosen (KState.flags); the one not chosen exits.
//   1  the exact fp32 pass.  It also writes its iterate to a.gbase (the base G of later
//      corrections) and, where kFlagWriteShadow is set, stores the tile it holds as bf16 (the
//      bits of pack.hip's rounding) into a.shadow: bf16 panels of the fp32 chunk's own width,
//      fp32 chunk ch = shadow panel ch.
//   2  the correction pass on the bf16 shadow (B16, PANEL).  a.coef holds c_k - c^b_k; phase A
//      is g' = G + sum_k (c_k - c^b_k) x~_k, phase B the row sums e_k = sum_j D_j x~_kj with
//      D = g' - G, and the finisher threads sum C = sum_j D_j (D_j + 2 G_j) into a third slab
//      value: ||x~_k - g'||^2 - ||x~_k - G||^2 = C - 2 e_k, which the K-space step adds to the
//      base pass's exact distances.
template <int V, int NW, int LPR, int R, int MODE, int SCHED, int OCC = 1, bool PANEL = false,
          bool B16 = false, bool SELF = false, int DELTA = 0>
__global__ void __launch_bounds__(NW * 64, OCC * NW / 4) weiszfeld_pass(PassArgs a) {
  static_assert(!SELF || MODE == 0, "the old iterate as column term: STEP passes only");
  static_assert(DELTA == 0 || (MODE == 0 && PANEL && !SELF), "DELTA: gm2 STEP on panels");
  static_assert(DELTA != 1 || (!B16 && V == 4), "the shadow is written from the fp32 tile");
  static_assert(DELTA != 2 || (B16 && SCHED == 0), "the correction pass reads the bf16 shadow");
  constexpr bool PIPE = SCHED == 1, ROLL = SCHED == 2 || SCHED == 3, ROLL2 = SCHED == 3;
  constexpr bool SUM_ONLY = MODE == 3;     // closing pass of the Gram variant: g = sum c_k x_k
  constexpr bool OMA_INIT = MODE == 4;
  constexpr bool INIT = MODE == 1 || MODE == 2 || OMA_INIT;
  constexpr bool WANT_R = MODE == 2;
  static_assert(!OMA_INIT || V == 4, "fused OMA: one Philox block per float4 group");
  static_assert(!B16 || (!SUM_ONLY && !OMA_INIT && !PIPE && !ROLL2), "bf16: modes 0-2, SCHED 0 / 2");
  constexpr int ES = B16 ? 2 : 4;          // bytes per element of X
  constexpr int QW = 64 / LPR;
  constexpr int NRG = NW * QW;
  constexpr int J = LPR * V;
  constexpr int RPL = R > LPR ? R / LPR : 1;
  static_assert(J <= NW * 64, "one finisher thread per column");
  using T = Tile<V, R, B16, DELTA == 2>;
  constexpr int NFIN = DELTA == 2 ? 3 : 2;

  typedef typename std::conditional<SELF, double, float>::type red_t;   // SELF: phase A in fp64
  __shared__ red_t s_red[NW][J];
  __shared__ float s_g[INIT ? 2 : 1][J];   // INIT: by chunk parity (one barrier per chunk)
  __shared__ double s_fin[NFIN][NW];
  __shared__ float s_w[OCC > 1 ? NW * QW * R : 1];

  if (gridDim.y > 1) {                       // batched independent problems
    const int64_t pb = blockIdx.y;
    a.X += pb * a.x_ps;
    a.g_old += pb * a.gold_ps;
    if (a.g_new) a.g_new += pb * a.gnew_ps;
    a.coef += pb * a.K;
    a.st += pb;
    a.slab += pb * (int64_t)gridDim.x * a.slab_stride;
    a.seed += (uint64_t)pb * kSeedStride;
    a.oma_seed += (uint64_t)pb * kSeedStride;
  }
  if (!SUM_ONLY && a.st->done) return;
  bool wr_shadow = false;
  (void)wr_shadow;
  if constexpr (DELTA != 0) {
    const uint32_t fl = a.st->flags;
    if (((fl & kFlagNextDelta) != 0) != (DELTA == 2)) return;
    wr_shadow = DELTA == 1 && (fl & kFlagWriteShadow) != 0;
  }

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane % LPR, q = lane / LPR;
  const int rg = w * QW + q;
  const int64_t K = a.K, d = a.d;
  const int64_t nch = (d + J - 1) / J;
  const int64_t grid = gridDim.x;

  // Row r of this thread = wave-uniform row-group base (SGPRs) + ONE 32-bit lane
  // offset shared by all R rows (measured 1.8 % faster than buffer_load with one
  // shared VGPR offset on the C3 pass: 6.90 vs 7.03 ms, same box;
  // profiles/history/r02_ab_loads.txt).
  bool rval[R];
#pragma unroll
  for (int i = 0; i < R; ++i) rval[i] = rg + (int64_t)NRG * i < K;
  typedef typename std::conditional<B16, uint16_t, float>::type elem;
  const elem* const Xe = reinterpret_cast<const elem*>(a.X);
  const elem* base[R];
#pragma unroll
  for (int i = 0; i < R; ++i) base[i] = Xe + (int64_t)(w * QW + NRG * i) * a.ldx;
  const uint32_t goff = (uint32_t)q * (uint32_t)a.ldx;
  const uint32_t poff = ((uint32_t)q * J + (uint32_t)(c * V)) * ES;   // PANEL: bytes from the wave's rows

  // fused OMA: this thread's rows' equalisation scales sd / |h_k| (row k keyed as in
  // the standalone OMA kernel)
  float osc[OMA_INIT ? R : 1];
  if constexpr (OMA_INIT) {
#pragma unroll
    for (int i = 0; i < R; ++i)
      osc[i] = rval[i] ? oma_row_scale(a.oma_seed, (uint64_t)(rg + NRG * i), a.oma_sd) : 0.f;
  }
  float wt[OCC > 1 ? 1 : R];
  float a_noise = 0.f;
  if constexpr (!INIT) {
    if constexpr (OCC > 1) {
      for (int k = tid; k < NRG * R; k += NW * 64) s_w[k] = k < K ? a.coef[k] : 0.f;
      __syncthreads();
    } else {
#pragma unroll
      for (int i = 0; i < R; ++i) wt[i] = rval[i] ? a.coef[rg + NRG * i] : 0.f;
    }
    a_noise = a.st->a_noise;
  }

  // bf16: the two columns of packed word j of row i, widened.  The arithmetic on them is
  // written on the pair, so that it compiles to v_pk_fma_f32 / v_pk_add_f32: per column the
  // same fmaf as the fp32 tile's, two columns per instruction (18 % fewer VALU instructions
  // in the K <= 1024 STEP kernel than widening and accumulating column by column)
  typedef float f2 __attribute__((ext_vector_type(2)));
  auto xpair = [](const T& t, int i, int j) -> f2 {
    const uint32_t p = (uint32_t)t.x[i][j];
    return f2{__uint_as_float(p << 16), __uint_as_float(p & 0xffff0000u)};
  };
  auto zero_col = [](T& t, int i, int v) {
    if constexpr (B16) t.x[i][v >> 1] &= (v & 1) ? 0x0000ffffu : 0xffff0000u;
    else t.x[i][v] = 0.f;
  };
  auto fetch_row = [&](int64_t ch, T& t, int i) {
    if constexpr (PANEL) {
      // One buffer resource per (chunk, row group i) in SGPRs, sized to the rows
      // that exist (rows >= K read 0 through the range check), + the one lane
      // offset (columns >= d: an out-of-range offset).  Branch-free.
      constexpr int64_t GB = (int64_t)NRG * J * ES;   // bytes per row group
      const int64_t wb = (int64_t)(w * QW) * J * ES + i * GB;   // this wave's rows, bytes
      const int64_t nrec = (int64_t)K * J * ES - wb;
      const uint32_t vo = (ch < nch && ch * J + c * V < d) ? poff : 0x80000000u;
      load_rows<B16 ? 4 : V>(reinterpret_cast<const typename T::word*>(
                                 reinterpret_cast<const char*>(Xe + ch * a.panel_stride) + wb),
                             vo, t.x[i], nrec <= 0 ? 0 : nrec > 0x7fffffff ? 0x7fffffff : (int)nrec);
      // last chunk (block-uniform): padding columns read as 0 (bf16: in zero_padding,
      // once per chunk, so that the rolled loads stay one straight line)
      if (!B16 && (ch + 1) * J > d) {
#pragma unroll
        for (int v = 0; v < V; ++v)
          if (ch * J + c * V + v >= d) zero_col(t, i, v);
      }
      return;
    }
    const int64_t col = ch * J + (int64_t)c * V;
    const bool cval = ch < nch && col < d;   // V | d: a lane's group is all-in or all-out
    if (cval && rval[i]) {
      load_cols<B16 ? 4 : V>(reinterpret_cast<const typename T::word*>(
                                 base[i] + (goff + (uint32_t)col)), t.x[i]);
    } else {
#pragma unroll
      for (int v = 0; v < (B16 ? V / 2 : V); ++v) t.x[i][v] = 0;
    }
  };
  // bf16 panels: the last chunk's padding columns, masked out of the packed words when the
  // chunk is processed (never trusted: ClientPanels zero-fills them, a caller's buffer may not)
  auto zero_padding = [&](int64_t ch, T& t) {
    if constexpr (B16 && PANEL) {
      if ((ch + 1) * J > d) {
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
          for (int v = 0; v < V; ++v)
            if (ch * J + c * V + v >= d) zero_col(t, i, v);
      }
    }
  };
  // The column-wise operands ride with the chunk on the J finisher threads (one
  // register each), not on every lane: INIT then costs the registers STEP does,
  // and both take the rolling prefetch without spilling.
  auto fetch_aux = [&](int64_t ch, T& t) {
    const int64_t gj = ch * J + tid;
    const bool fin = tid < J && ch < nch && gj < d;
    t.gold = fin ? a.g_old[gj] : 0.f;
    if constexpr (!INIT) t.hn = (fin && a.noise == 2) ? a.hnoise[gj] : 0.f;
    if constexpr (DELTA == 2) t.gb = fin ? a.gbase[gj] : 0.f;
  };
  auto fetch = [&](int64_t ch, T& t) {
#pragma unroll
    for (int i = 0; i < R; ++i) fetch_row(ch, t, i);
    fetch_aux(ch, t);
  };

  double row_acc[RPL], row_acc2[RPL];
#pragma unroll
  for (int m = 0; m < RPL; ++m) row_acc[m] = row_acc2[m] = 0.0;
  double mv_acc = 0.0, gn_acc = 0.0, cg_acc = 0.0;

  // ROLL: row i of chunk `nxt` is loaded into t.x[i] as soon as phase B has
  // consumed row i of chunk ch, so the next chunk's loads are in flight during
  // phase B, the row reductions and the next chunk's barriers (no second tile).
  int par = 0;   // INIT: chunk parity -> s_g buffer
  // fused OMA: noise the tile's real elements (element (k, global column c) takes normal
  // c & 3 of the Philox block (row k, c >> 2): V = 4 columns = one block) and write them
  // back where they were read; padding columns and rows are left untouched
  // (a generic lambda: its body is only instantiated for MODE 4, fp32 tiles)
  auto oma_tile = [&](int64_t ch, auto& t) {
    const int64_t col = ch * J + (int64_t)c * V;
    if (ch >= nch || col >= d) return;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (!rval[i]) continue;
      const int64_t k = rg + (int64_t)NRG * i;
      float z[4];
      normal4_hw(a.oma_seed, kStreamOmaNoise, (uint64_t)k, (uint64_t)(a.col_off + col) >> 2, z);
      // (the padding columns of a partial last group stay 0: they enter the distances)
#pragma unroll
      for (int v = 0; v < V; ++v)
        if (col + v < d) t.x[i][v] = oma_noisy(t.x[i][v], osc[i], z[v]);
      float* dst;
      if constexpr (PANEL)
        dst = const_cast<float*>(a.X) + ch * a.panel_stride + k * J + c * V;
      else
        dst = reinterpret_cast<float*>(const_cast<elem*>(base[i])) + goff + col;
      if (col + V <= d) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<f4*>(dst) = f4{t.x[i][0], t.x[i][1], t.x[i][2], t.x[i][3]};
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v)
          if (col + v < d) dst[v] = t.x[i][v];
      }
    }
  };
  // DELTA = 1: the fp32 tile of chunk ch, rounded to bf16 (to nearest even, NaN -> 0x7FC0: the
  // bits pack.hip produces), into shadow panel ch, a panel of the fp32 chunk's own width: 8 bytes
  // per lane and row, rows J * 2 bytes apart, so a wave instruction writes QW whole adjacent
  // rows and a block one contiguous K * J * 2 bytes.  (Two fp32 chunks per 64-column bf16 panel,
  // 64-byte halves of 128-byte rows written by different blocks at different times, made the
  // writing pass 16.0 ms against 6.3 ms for the plain pass at C3: DESIGN.md §3.1.)  Padding
  // columns are 0 in the tile and are stored as 0; rows >= K are not stored (the buffer holds
  // ceil(d / J) whole panels of K rows).
  auto store_shadow = [&](int64_t ch, const auto& t) {
    auto rne = [](float f) -> uint32_t {
      const uint32_t u = __float_as_uint(f);
      return f != f ? 0x7fc0u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    };
    // as the loads: one buffer resource per row group in SGPRs, sized to the rows that exist
    // (a store to a row >= K is dropped by the range check), + one lane offset
    constexpr int RB = J * 2;                         // bytes per row of a shadow panel
    char* const pan = reinterpret_cast<char*>(a.shadow + ch * a.shadow_stride);
    const uint32_t vo = (uint32_t)(q * RB + c * V * 2);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t wb = (int64_t)(w * QW + NRG * i) * RB;
      const int64_t nrec = (int64_t)K * RB - wb;
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          pan + wb, 0, nrec <= 0 ? 0 : (int)nrec, 0x00020000);
      typedef uint32_t u2 __attribute__((ext_vector_type(2)));
      const u2 o = u2{rne(t.x[i][0]) | rne(t.x[i][1]) << 16, rne(t.x[i][2]) | rne(t.x[i][3]) << 16};
      __builtin_amdgcn_raw_buffer_store_b64(o, rs, vo, 0, 0);
    }
  };
  auto process = [&](int64_t ch, T& t, int64_t nxt) {
    float gv[V];
    zero_padding(ch, t);
    if constexpr (DELTA == 1) {
      if (wr_shadow) store_shadow(ch, t);
    }
    if constexpr (OMA_INIT) oma_tile(ch, t);
    if constexpr (INIT) {
      // the guess at this chunk's columns -> LDS (buffer by parity: a thread still
      // reading the previous chunk's buffer has not passed this chunk's barrier)
      if (tid < J) {
        s_g[par][tid] = t.gold;
        gn_acc += (double)(t.gold * t.gold);
      }
      __syncthreads();
#pragma unroll
      for (int v = 0; v < V; ++v) gv[v] = s_g[par][c * V + v];
      par ^= 1;
    } else {
      // phase A: weighted column sums over this thread's rows ...
      // SELF (centered clipping) sums in fp64, products included: with v' = sum_k c_k x_k + a v
      // and sum c + a = 1, identical rows x_k = v must give v back, and an fp32 sum of K terms
      // c_k v is 3-6 ulp off at K = 50-1024 whatever the coefficients are (measured); the
      // fp64 sum is exact to 2^-53 K and the one rounding left is the final conversion.
      float acc[V];
      f2 accp[B16 ? V / 2 : 1];   // bf16: the column pairs' sums
      red_t accd[SELF ? V : 1];
      if constexpr (SELF) {
#pragma unroll
        for (int v = 0; v < V; ++v) accd[v] = 0;
      }
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = 0.f;
#pragma unroll
      for (int j = 0; j < (B16 ? V / 2 : 1); ++j) accp[j] = f2{0.f, 0.f};
#pragma unroll
      for (int i = 0; i < R; ++i) {
        float wi;
        if constexpr (OCC > 1) wi = s_w[rg + NRG * i];
        else wi = wt[i];
        if constexpr (B16) {
#pragma unroll
          for (int j = 0; j < V / 2; ++j) {
            const f2 xv = xpair(t, i, j);
            if constexpr (SELF) {
              accd[2 * j] = fma((double)wi, (double)xv[0], accd[2 * j]);
              accd[2 * j + 1] = fma((double)wi, (double)xv[1], accd[2 * j + 1]);
            } else {
              accp[j] = __builtin_elementwise_fma(f2{wi, wi}, xv, accp[j]);
            }
          }
        } else {
#pragma unroll
          for (int v = 0; v < V; ++v) {
            if constexpr (SELF) accd[v] = fma((double)wi, (double)t.x[i][v], accd[v]);
            else acc[v] = fmaf(wi, t.x[i][v], acc[v]);
          }
        }
      }
      if constexpr (B16) {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = accp[v >> 1][v & 1];
      }
      // ... over the wave's row groups ...
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if constexpr (SELF) accd[v] += __shfl_xor(accd[v], o, 64);
          else acc[v] += __shfl_xor(acc[v], o, 64);
        }
      if (q == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if constexpr (SELF) s_red[w][c * V + v] = accd[v];
          else s_red[w][c * V + v] = acc[v];
        }
      }
      __syncthreads();
      // ... and over the waves: one finisher thread per column writes g'.
      if (tid < J) {
        red_t sum = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) sum += s_red[ww][tid];
        const int64_t gj = ch * J + tid;
        float gnew = 0.f;
        if (gj < d) {
          if constexpr (!SELF) gnew = sum;
          if (a.noise == 1) {
            gnew = fmaf(a_noise, normal1(a.seed, kStreamNoise, a.iter, a.col_off + gj), gnew);
          } else if (a.noise == 2) {
            gnew = fmaf(a_noise, t.hn, gnew);
          }
          // centered clipping: the old iterate's share a = 1 - sum_k c_k (already here as gold)
          if constexpr (SELF) gnew = (float)fma((double)a_noise, (double)t.gold, (double)sum);
          if constexpr (DELTA == 2) gnew = t.gb + sum;
          a.g_new[gj] = gnew;
          if constexpr (DELTA == 1) a.gbase[gj] = gnew;
          const float diff = t.gold - gnew;
          mv_acc += (double)(diff * diff);
          gn_acc += (double)(gnew * gnew);
        }
        if constexpr (DELTA == 2) {
          // phase B's column operand is the displacement of the STORED iterate from the base
          const float dj = gj < d ? gnew - t.gb : 0.f;
          cg_acc += (double)dj * ((double)dj + 2.0 * (double)t.gb);
          gnew = dj;
        }
        s_g[0][tid] = gnew;
      }
      __syncthreads();
#pragma unroll
      for (int v = 0; v < V; ++v) gv[v] = s_g[0][c * V + v];
    }
    if constexpr (SUM_ONLY) {
      if constexpr (ROLL) fetch(nxt, t);
      return;
    }
    if constexpr (B16 && !INIT) {
      // phase B widens the packed tile again.  The empty asm makes the packed words opaque:
      // without it the compiler reuses phase A's widened values and keeps them, an fp32
      // tile of twice the registers, alive across the barriers (spills).
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int v = 0; v < V / 2; ++v) asm volatile("" : "+v"(t.x[i][v]));
    }
    // phase B: squared distances of this thread's rows to the (new) iterate
    // (+ ||x_k||^2 for the AirComp INIT pass).
    float e[R], e2[WANT_R ? R : 1];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      float s = 0.f, s2 = 0.f;
      if constexpr (B16) {
        // even and odd columns summed apart, then added
        f2 sp = f2{0.f, 0.f}, sp2 = f2{0.f, 0.f};
#pragma unroll
        for (int j = 0; j < V / 2; ++j) {
          const f2 xv = xpair(t, i, j);
          if constexpr (DELTA == 2) {
            sp = __builtin_elementwise_fma(xv, f2{gv[2 * j], gv[2 * j + 1]}, sp);
            continue;
          }
          const f2 tt = xv - f2{gv[2 * j], gv[2 * j + 1]};
          sp = __builtin_elementwise_fma(tt, tt, sp);
          if constexpr (WANT_R) sp2 = __builtin_elementwise_fma(xv, xv, sp2);
        }
        s = sp[0] + sp[1];
        s2 = sp2[0] + sp2[1];
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float tt = t.x[i][v] - gv[v];
          s = fmaf(tt, tt, s);
          if constexpr (WANT_R) s2 = fmaf(t.x[i][v], t.x[i][v], s2);
        }
      }
      e[i] = s;
      if constexpr (WANT_R) e2[i] = s2;
      if constexpr (ROLL) {
        // keep row i's next load behind row i's use: without the fence the
        // compiler hoists all R loads above phase B (two live tiles, spills)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
        fetch_row(nxt, t, i);
      }
    }
    if constexpr (ROLL) fetch_aux(nxt, t);
    transpose_reduce<LPR, R>(e, c);
#pragma unroll
    for (int m = 0; m < RPL; ++m) row_acc[m] += (double)e[m];
    if constexpr (WANT_R) {
      transpose_reduce<LPR, R>(e2, c);
#pragma unroll
      for (int m = 0; m < RPL; ++m) row_acc2[m] += (double)e2[m];
    }
  };

  if constexpr (PIPE) {
    T ta, tb;
    int64_t ch = blockIdx.x;
    fetch(ch, ta);
    for (; ch < nch; ch += 2 * grid) {
      fetch(ch + grid, tb);
      process(ch, ta, -1);
      if (ch + grid >= nch) break;       // block-uniform
      fetch(ch + 2 * grid, ta);
      process(ch + grid, tb, -1);
    }
  } else if constexpr (ROLL2) {
    // two tiles, each rolled two grid strides ahead: chunks c+1 and c+2 in flight while
    // c is reduced (for passes whose blocks are latency-bound on too few bytes in flight:
    // small chunks, C5's K = 50 x 128 panels)
    T ta, tb;
    int64_t ch = blockIdx.x;
    fetch(ch, ta);
    fetch(ch + grid, tb);
    for (; ch < nch; ch += 2 * grid) {
      process(ch, ta, ch + 2 * grid);
      if (ch + grid >= nch) break;       // block-uniform
      process(ch + grid, tb, ch + 3 * grid);
    }
  } else if constexpr (ROLL) {
    T t;
    fetch(blockIdx.x, t);
    for (int64_t ch = blockIdx.x; ch < nch; ch += grid) process(ch, t, ch + grid);
  } else {
    for (int64_t ch = blockIdx.x; ch < nch; ch += grid) {
      T t;
      fetch(ch, t);
      process(ch, t, -1);
    }
  }

  // Per-block partials -> slab row.  [D2 (K)] [r (K), INIT only] [mv2] [gn2];
  // the Gram closing pass (SUM_ONLY) writes [||p - g||^2] [||g||^2] only.
  double* out = a.slab + (int64_t)blockIdx.x * a.slab_stride;
  const int i_c = row_of_lane<LPR, R>(c);
  constexpr int SPAN = R < LPR ? LPR / R : 1;   // lanes holding copies of one row sum
  if (!SUM_ONLY && (c % SPAN) == 0) {
#pragma unroll
    for (int m = 0; m < RPL; ++m) {
      const int64_t k = rg + (int64_t)NRG * (i_c + m);
      if (k < K) {
        out[k] = row_acc[m];
        if constexpr (INIT) out[K + k] = row_acc2[m];
      }
    }
  }
  if constexpr (DELTA != 0) {
    // the two kinds run on grids of their own and one slab_reduce sums a.slab_rows rows: the
    // rows only the other kind's larger grid would fill are zeros
    for (int64_t r = blockIdx.x + grid; r < a.slab_rows; r += grid)
      for (int64_t k2 = tid; k2 < a.slab_stride; k2 += NW * 64) a.slab[r * a.slab_stride + k2] = 0.0;
  }
  const double mv = wave_sum(mv_acc), gn = wave_sum(gn_acc);
  if (lane == 0) {
    s_fin[0][w] = mv;
    s_fin[1][w] = gn;
  }
  if constexpr (DELTA == 2) {
    const double cg = wave_sum(cg_acc);
    if (lane == 0) s_fin[2][w] = cg;
  }
  __syncthreads();
  if (tid == 0) {
    double m = 0.0, g = 0.0;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {
      m += s_fin[0][ww];
      g += s_fin[1][ww];
    }
    const int64_t b = SUM_ONLY ? 0 : INIT ? 2 * K : K;
    out[b] = m;
    out[b + 1] = g;
    if constexpr (DELTA == 2) {
      double cg = 0.0;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) cg += s_fin[2][ww];
      out[b + 2] = cg;
    }
  }
}

}  // namespace gmk
