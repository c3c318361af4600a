// sp_net_rows.hip -- the superpoint stage's deform network evaluated on P rows (every Gaussian), as fp32 MFMA row blocks.
//
// Stages `init_fix` / `init` (the first 10 k of the reference's 80 k default steps, exps/default.yaml:12-19) call the SAME
// DeformNetwork (sk_gs.py:209-315) that sp_mlp.hip runs on the 512 superpoints, on all P Gaussians: `sp_deform_net(x, t)` with
// gradients and again under no_grad (init_stage, sk_gs.py:741-749), `canonical_net(points_c, t)` with gradients (the c_net loss,
// sk_gs.py:1501-1508,1535-1536), and 16-17 no-grad forwards in init_superpoints (sk_gs.py:678-690).  P grows from 2 000 to
// ~100 k.  One row costs 508 928 multiply-adds forward and 970 240 backward (with the weight gradients): dense GEMM work.
// sp_mlp.hip's shape (4 rows per workgroup, the 2 MB of weights re-streamed per block, 8.6 KB of activations per row kept in a
// runner per row count) is the wrong one for P rows; these kernels are the GEMM shape:
//
//   forward    a workgroup carries 64 rows through the 8 layers and the heads (v_mfma_f32_32x32x2_f32: exact f32).  The
//              activations stay in LDS between layers ([64][256], in place); every layer's weights stream through LDS in
//              chunks of 16 contraction columns x 256 outputs (double-buffered, the next chunk in registers while the current
//              one is multiplied), shared by the 8 waves (wave w: rows 32 (w & 1) .., outputs 64 (w >> 1) ..).  The time input
//              is the same in every row, so its columns of layers 0 and 5 fold into those layers' biases:
//                  cb_l = b_l + W_l[:, 63:63 + tw] t_emb       (l = 0, 5; tw = 30, or 1 + 2 degree with the raw time encoding)
//              and the encoded input x0 is freq(x, 10) alone, 63 columns padded to 64.  The time network (13 -> 256 -> 30,
//              11 k multiply-adds) and the folds (15 k) run in the prologue of every workgroup: per 64-row block, not per row.
//              With a saved buffer the forward also writes x0 [Pp][64] and every layer's output Y_l [Pp][256] (8448 B per row).
//   backward A the same row blocks walk back: gZ_7 = (g_raw W_heads) * (Y_7 > 0), then gZ_{l-1} = (gZ_l W_l[:, hidden]) *
//              (Y_{l-1} > 0) for l = 7 .. 1, the weights streamed in chunks of 16 OUTPUT rows (transposed into LDS).  Every gZ_l
//              goes to the workspace.
//   backward B the weight gradients gW_l = gZ_l^T X_l are a reduction over the P rows: 124 tiles of 64 x 64 (layer 0 and
//              layer 5's input part over x0, the hidden parts over Y_{l-1}, the heads over Y_7) times S row splits (S from P
//              alone), one wave per (tile, split), each writing its partial tile; bias gradients are the column sums of gZ
//              taken by the tiles at input column 0.
//   backward C the partials summed over the splits in split order (no float atomics: the same inputs give the same bits),
//              written into the gradient tensors; one workgroup sums the bias gradients, one the time columns and the time
//              network: gW_l[:, 63:63 + tw] = gb_l t_emb (l = 0, 5), d loss / d t_emb = gb_0 W_0[:, 63:93] + gb_5 W_5[:, 63:93]
//              (the trick of sp_mlp.hip), then the two timenet layers.
// No gradient w.r.t. the positions or the time: every caller detaches them (sk_gs.py:746-748).
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "skgs_common.h"

namespace skgs {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int W_     = 256;  // layer width
constexpr int NL     = 8;    // hidden layers
constexpr int SKIP   = 4;    // after this layer the encoded input is concatenated in front (layer 5 reads [x_emb | t_emb | h])
constexpr int PDIM   = 63;   // freq(x, 10)
constexpr int XC     = 64;   // x0 columns (63 + one zero)
constexpr int TDIM   = 13;   // freq(t, 6): the time network's input
constexpr int THID   = 256, TOUT = 30;
constexpr int BM     = 64;   // rows per workgroup of the row-block launches
constexpr int NT     = 512;  // 8 waves
constexpr int KC     = 16;   // contraction columns per weight chunk
constexpr int BP     = KC + 4;   // LDS pitch of a chunk row (floats): 5 i mod 16 distinct 16-B slots for 32 lanes' ds_read_b128
constexpr int HP     = W_ + 4;   // ... of an activation row: 260 = 4 mod 64
constexpr int XP     = XC + 4;   // ... of an x0 row
constexpr int NOUT_MAX = 14;
constexpr int HDR    = 512;  // saved header (floats): freq(t) [32] | time hidden [256] | t_emb [32]
constexpr int NTILE  = 4 + 7 * 16 + 4 + 4;  // weight-gradient tiles: layer 0 | hidden parts of layers 1-7 | layer 5 over x0 | heads
constexpr int NBIAS  = NL + 1;              // bias-gradient partial rows per split: layers 0-7, heads
constexpr int SPLIT_ROWS = 1024, MAX_SPLITS = 64;

__host__ __device__ inline size_t pad_rows(int P) { return ((size_t) P + BM - 1) / BM * BM; }
__host__ __device__ inline int n_splits(int P) {  // row splits of the weight gradients: a function of P alone
  const size_t s = pad_rows(P) / SPLIT_ROWS;
  return s < 1 ? 1 : (s > MAX_SPLITS ? MAX_SPLITS : (int) s);
}
__host__ __device__ inline int split_rows(int P) {  // rows of one split, a multiple of 16
  const size_t per = (pad_rows(P) + n_splits(P) - 1) / n_splits(P);
  return (int) ((per + 15) / 16 * 16);
}

struct SavedView {
  float* tenc;  // [32]  freq(t) (13, or 1 + 2 degree, used)
  float* thid;  // [256] the time network's hidden layer (post-ReLU)
  float* temb;  // [32]  t_emb, what layers 0 and 5 read
  float* x0;    // [Pp][64]
  float* Y;     // [NL][Pp][256]
};
__host__ __device__ inline size_t saved_floats(int P) { return HDR + pad_rows(P) * (XC + (size_t) NL * W_); }
__host__ __device__ inline SavedView saved_view(void* base, int P) {
  float* p = reinterpret_cast<float*>(base);
  SavedView v;
  v.tenc = p, v.thid = p + 32, v.temb = p + 32 + THID;
  v.x0 = p + HDR;
  v.Y  = v.x0 + pad_rows(P) * XC;
  return v;
}
struct WorkView {
  float* GH;    // [Pp][16]  head cotangents (zero beyond nout and beyond P)
  float* GZ;    // [NL][Pp][256]
  float* PART;  // [S][NTILE][64 * 64]
  float* GBP;   // [S][NBIAS][256]
};
__host__ __device__ inline size_t work_floats(int P) {
  const size_t Pp = pad_rows(P), S = n_splits(P);
  return Pp * 16 + (size_t) NL * Pp * W_ + S * NTILE * 4096 + S * NBIAS * W_;
}
__host__ __device__ inline WorkView work_view(void* base, int P) {
  const size_t Pp = pad_rows(P), S = n_splits(P);
  WorkView v;
  v.GH   = reinterpret_cast<float*>(base);
  v.GZ   = v.GH + Pp * 16;
  v.PART = v.GZ + (size_t) NL * Pp * W_;
  v.GBP  = v.PART + S * NTILE * 4096;
  return v;
}

struct NetPtrs {
  const float* points;
  const float* time;
  const float *tw1, *tb1, *tw2, *tb2;  // NULL with the raw time encoding
  const float* W[NL];
  const float* b[NL];
  const float* head_w[4];  // warp (3), rotation (4), scaling (3), local rotation (4): the order of the raw output row
  const float* head_b[4];
  int nout, in0, tw, tdim;  // tw: t_emb columns (30, or tdim); tdim: freq(t) columns (13, or 1 + 2 degree)
};
struct GradPtrs {
  float *tw1, *tb1, *tw2, *tb2;
  float* W[NL];
  float* b[NL];
  float* head_w[4];
  float* head_b[4];
};
__host__ __device__ inline int layer_ld(int l, int in0) { return l == 0 ? in0 : (l == SKIP + 1 ? in0 + W_ : W_); }
__host__ __device__ inline int layer_hofs(int l, int in0) { return l == SKIP + 1 ? in0 : 0; }
__device__ __forceinline__ int head_of(int o, int& row) {  // raw output column -> (head, row of that head's matrix)
  if (o < 3) return row = o, 0;
  if (o < 7) return row = o - 3, 1;
  if (o < 10) return row = o - 7, 2;
  return row = o - 10, 3;
}
template <class T, int N>
__device__ __forceinline__ T pick(T const (&p)[N], int k) {  // p[k] by selects (a dynamic index into a kernel argument goes to scratch)
  T r = p[0];
#pragma unroll
  for (int j = 1; j < N; ++j) r = k == j ? p[j] : r;
  return r;
}

struct __attribute__((packed, aligned(4))) f4u {  // a float4 at 4-byte alignment (weight rows of 93 / 349 floats)
  float x, y, z, w;
};
__device__ __forceinline__ float4 ldg4(const float* p) {
  const f4u v = *reinterpret_cast<const f4u*>(p);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
  for (int q = 0; q < 16; ++q) a[q] = 0.f;
}

// ---- one wave's product of a 32-row A tile with two 32-column B tiles over NK contraction columns (NK / 8 sub-steps) -------
// v_mfma_f32_32x32x2_f32: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31].  The contraction order inside 8
// columns is permuted so that each operand is ONE ds_read_b128: lane half h reads columns 4 h .. 4 h + 3 of its row, step e of
// the four MFMAs takes element e -- A and B agree on the column (4 h + e), and a sum does not care about the order.
// ap: &A[row 32 rt + i][k0 + 4 h], bp: &B[output 64 cg + i][k0 + 4 h] (B rows are the OUTPUTS, contraction contiguous).
template <int NK, int BPITCH>
__device__ __forceinline__ void mma_rows(f32x16 (&acc)[2], const float* ap, const float* bp) {
#pragma unroll
  for (int s = 0; s < NK / 8; ++s) {
    const float4 a  = *reinterpret_cast<const float4*>(ap + 8 * s);
    const float4 b0 = *reinterpret_cast<const float4*>(bp + 8 * s);
    const float4 b1 = *reinterpret_cast<const float4*>(bp + 32 * BPITCH + 8 * s);
    acc[0] = mfma32(a.x, b0.x, acc[0]), acc[1] = mfma32(a.x, b1.x, acc[1]);
    acc[0] = mfma32(a.y, b0.y, acc[0]), acc[1] = mfma32(a.y, b1.y, acc[1]);
    acc[0] = mfma32(a.z, b0.z, acc[0]), acc[1] = mfma32(a.z, b1.z, acc[1]);
    acc[0] = mfma32(a.w, b0.w, acc[0]), acc[1] = mfma32(a.w, b1.w, acc[1]);
  }
}
// accumulator register q of lane l: row (q & 3) + 8 (q >> 2) + 4 (l >> 5) of the 32-row tile, column l & 31
__device__ __forceinline__ int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// the time input of every row: freq(t), the time network, t_emb -> s_t [tenc 32 | thid 256 | temb 32]; then the folded biases
// cb_0, cb_5 -> rows 0 and 5 of s_bias [8][256].  Every thread of the 512 reaches the barriers.
__device__ __forceinline__ void time_prologue(const NetPtrs& n, float* s_t, float* s_bias, const SavedView& sv, int save) {
  const int tid = threadIdx.x;
  float* s_tenc = s_t;
  float* s_thid = s_t + 32;
  float* s_temb = s_t + 32 + THID;
  if (tid < 32) {
    float v = 0.f;
    if (tid < n.tdim) {
      const float t = n.time[0];
      v = t;
      if (tid >= 1) {
        const int col = tid - 1;
        v = sinf(scalbnf(t, col / 2) + (float) (col % 2) * (3.141592653589793f / 2));
      }
    }
    s_tenc[tid] = v;
    if (!n.tw1) s_temb[tid] = v;  // raw time encoding: t_emb IS freq(t)
  }
  __syncthreads();
  if (n.tw1) {
    if (tid < THID) {
      float h = n.tb1[tid];
#pragma unroll
      for (int k = 0; k < TDIM; ++k) h += n.tw1[tid * TDIM + k] * s_tenc[k];
      s_thid[tid] = fmaxf(h, 0.f);
    }
    __syncthreads();
    if (tid < TOUT * 8) {
      const int o = tid >> 3, part = tid & 7;
      float v = 0.f;
      for (int k = part; k < THID; k += 8) v += n.tw2[o * THID + k] * s_thid[k];
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      if (part == 0) s_temb[o] = v + n.tb2[o];
    } else if (tid >= 256 && tid < 258) {
      s_temb[TOUT + tid - 256] = 0.f;
    }
    __syncthreads();
  }
  if (save && blockIdx.x == 0) {  // the whole header (its unused tail zero): same inputs, same saved bytes
    float v = 0.f;
    if (tid < 32) v = s_tenc[tid];
    else if (tid < 32 + THID) v = n.tw1 ? s_thid[tid - 32] : 0.f;
    else if (tid < 64 + THID) v = s_temb[tid - 32 - THID];
    sv.tenc[tid] = v;  // (tenc is the header's base; NT == HDR)
  }
  {  // cb_l = b_l + W_l[:, 63:63 + tw] t_emb: thread o (l = 0) or 256 + o (l = 5)
    const int l = tid < W_ ? 0 : SKIP + 1, o = tid & (W_ - 1);
    const float* w = (l == 0 ? n.W[0] : n.W[SKIP + 1]) + (size_t) o * layer_ld(l, n.in0) + PDIM;  // (selects, not a dynamic
    float v = (l == 0 ? n.b[0] : n.b[SKIP + 1])[o];                                                 //  index: that goes to scratch)
    for (int c = 0; c < n.tw; ++c) v += w[c] * s_temb[c];
    s_bias[l * W_ + o] = v;
  }
  __syncthreads();
}

// forward weight chunks: layer 0 has 4 (x0's 64 columns; column 63 is zero), layer 5 has 4 + 16, the others 16
__host__ __device__ constexpr int fwd_chunks(int l) { return l == 0 ? XC / KC : (l == SKIP + 1 ? (XC + W_) / KC : W_ / KC); }

// chunk c of layer l into registers: thread element e = tid + 512 u: output j = e >> 2, columns 16 c + 4 (e & 3) ..
__device__ __forceinline__ void fwd_load(const NetPtrs& n, int l, int c, float4 (&pf)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = threadIdx.x + NT * u, j = e >> 2, kv = KC * c + 4 * (e & 3);
    const int ld = layer_ld(l, n.in0);
    const float* row = pick(n.W, l) + (size_t) j * ld;
    float4 v;
    if (l == 0 || (l == SKIP + 1 && kv < XC)) {  // the x_emb columns; column 63 (a time column of W) is folded into the bias
      v = ldg4(row + kv);
      if (kv + 3 == XC - 1) v.w = 0.f;
    } else {
      v = ldg4(row + (l == SKIP + 1 ? n.in0 + kv - XC : kv));
    }
    pf[u] = v;
  }
}
__device__ __forceinline__ void fwd_store(float* bs, const float4 (&pf)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = threadIdx.x + NT * u;
    *reinterpret_cast<float4*>(bs + (e >> 2) * BP + 4 * (e & 3)) = pf[u];
  }
}

// LDS of the row-block launches (floats, one dynamic array)
constexpr int L_X0 = 0;                    // [64][XP]  x0 (forward)
constexpr int L_H  = L_X0 + BM * XP;       // [64][HP]  activations (forward) / gZ (backward)
constexpr int L_B  = L_H + BM * HP;        // [2][256][BP] weight chunks; the heads' [32][HP] image (forward)
constexpr int L_CB = L_B + 2 * W_ * BP;    // [8][256]  biases, rows 0 and 5 folded (forward)
constexpr int L_T  = L_CB + NL * W_;       // [320]     time (forward)
constexpr int L_GH = L_CB;                 // [64][16]  head cotangents (backward)
constexpr int L_HW = L_GH + BM * 16;       // [16][256] head weights (backward)
constexpr int L_END_F = L_T + 320;
constexpr int L_END_B = L_HW + 16 * W_;
static_assert(NT == HDR, "one thread per header float");
constexpr size_t ROWS_LDS_BYTES = (size_t) (L_END_F > L_END_B ? L_END_F : L_END_B) * 4;
static_assert(ROWS_LDS_BYTES <= 160 * 1024, "LDS");
static_assert(32 * HP <= 2 * W_ * BP, "head image fits the chunk buffers");

__global__ void __launch_bounds__(NT) sp_rows_forward_kernel(int P, NetPtrs n, float* __restrict__ raw, SavedView sv, int save) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_x0 = lds + L_X0;
  float* s_h  = lds + L_H;
  float* s_b  = lds + L_B;
  float* s_bias = lds + L_CB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int rt = wave & 1, cg = wave >> 1;
  const size_t r0 = (size_t) blockIdx.x * BM, Pp = pad_rows(P);
  // ---- the first weight chunk is on its way while the prologue runs
  float4 pf[2];
  fwd_load(n, 0, 0, pf);
  if (tid < W_) {  // the biases of layers 1-4, 6, 7 (0 and 5: folded by the prologue)
#pragma unroll
    for (int l = 1; l < NL; ++l)
      if (l != SKIP + 1) s_bias[l * W_ + tid] = n.b[l][tid];
  }
  time_prologue(n, lds + L_T, s_bias, sv, save);
  // ---- x0 = freq(x, 10) of the 64 rows (rows beyond P repeat the last one: computed, never written outside `saved`)
#pragma unroll
  for (int u = 0; u < BM * XC / NT; ++u) {
    const int e = tid + NT * u, row = e >> 6, c = e & 63;
    const size_t gr = r0 + row < (size_t) P ? r0 + row : (size_t) P - 1;
    float v = 0.f;
    if (c < 3) {
      v = n.points[3 * gr + c];
    } else if (c < PDIM) {
      const int col = c / 3 - 1, d = c % 3;
      v = sinf(scalbnf(n.points[3 * gr + d], col / 2) + (float) (col % 2) * (3.141592653589793f / 2));
    }
    s_x0[row * XP + c] = v;
    if (save) sv.x0[(r0 + row) * XC + c] = v;
  }
  fwd_store(s_b, pf);
  __syncthreads();
  // ---- the eight layers: one flat stream of weight chunks (120), the next one loaded while the current one is multiplied
  int buf = 0, nl = 0, nc = 1;  // the next chunk to load
  f32x16 acc[2];
#pragma unroll 1
  for (int l = 0; l < NL; ++l) {
    zero16(acc[0]), zero16(acc[1]);
    const int nch = fwd_chunks(l);
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
      const bool more = nl < NL;
      if (more) fwd_load(n, nl, nc, pf);
      const bool from_x0 = l == 0 || (l == SKIP + 1 && c < XC / KC);
      const float* ap = from_x0 ? s_x0 + (32 * rt + i) * XP + KC * c + 4 * h
                                : s_h + (32 * rt + i) * HP + KC * (l == SKIP + 1 ? c - XC / KC : c) + 4 * h;
      mma_rows<KC, BP>(acc, ap, s_b + buf * W_ * BP + (64 * cg + i) * BP + 4 * h);
      if (more) {
        fwd_store(s_b + (buf ^ 1) * W_ * BP, pf);
        if (++nc == fwd_chunks(nl)) nc = 0, ++nl;
      }
      __syncthreads();
      buf ^= 1;
    }
    // epilogue: bias, ReLU -> the next layer's input (in place: every wave is past its last read) and `saved`
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int o = 64 * cg + 32 * c + i;
      const float bb = s_bias[l * W_ + o];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 32 * rt + acc_row(q, h);
        const float v = fmaxf(acc[c][q] + bb, 0.f);
        s_h[row * HP + o] = v;
        if (save) sv.Y[((size_t) l * Pp + r0 + row) * W_ + o] = v;
      }
    }
    __syncthreads();
  }
  // ---- heads: raw [64][nout] = h W_heads^T + b.  The heads' rows as one [32][256] B image (rows >= nout zero); wave w: rows
  // 32 (w & 1) .., contraction quarter w >> 1; the four partial tiles meet in LDS
  float* s_hw = s_b;
  for (int e = tid; e < 32 * (W_ / 4); e += NT) {
    const int j = e >> 6, k4 = 4 * (e & 63);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < n.nout) {
      int hr;
      const int hd = head_of(j, hr);
      v = *reinterpret_cast<const float4*>(pick(n.head_w, hd) + (size_t) hr * W_ + k4);
    }
    *reinterpret_cast<float4*>(s_hw + j * HP + k4) = v;
  }
  __syncthreads();
  {
    const int kq = wave >> 1;
    f32x16 a1[2];
    zero16(a1[0]), zero16(a1[1]);
    // (one B tile: the second operand pointer of mma_rows reads rows 32 .. 63 of the image -- use the single-tile loop here)
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float4 a = *reinterpret_cast<const float4*>(s_h + (32 * rt + i) * HP + 64 * kq + 8 * s + 4 * h);
      const float4 b = *reinterpret_cast<const float4*>(s_hw + i * HP + 64 * kq + 8 * s + 4 * h);
      a1[s & 1] = mfma32(a.x, b.x, a1[s & 1]);
      a1[s & 1] = mfma32(a.y, b.y, a1[s & 1]);
      a1[s & 1] = mfma32(a.z, b.z, a1[s & 1]);
      a1[s & 1] = mfma32(a.w, b.w, a1[s & 1]);
    }
    __syncthreads();  // every wave is done with s_h: the partial tiles go there, [kq][64 rows][33]
    float* s_part = s_h;
#pragma unroll
    for (int q = 0; q < 16; ++q) s_part[(kq * BM + 32 * rt + acc_row(q, h)) * 33 + i] = a1[0][q] + a1[1][q];
  }
  __syncthreads();
  for (int e = tid; e < BM * n.nout; e += NT) {
    const int row = e / n.nout, j = e - row * n.nout;
    if (r0 + row >= (size_t) P) break;
    int hr;
    const int hd = head_of(j, hr);
    float v = pick(n.head_b, hd)[hr];
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) v += lds[L_H + (kq * BM + row) * 33 + j];
    raw[(r0 + row) * n.nout + j] = v;
  }
}

// =================================================================================================== backward, launch A
// chunk c of layer l transposed into registers: element e = tid + 512 u: output row 16 c + (e & 15), hidden columns 4 (e >> 4) ..
__device__ __forceinline__ void bwd_load(const NetPtrs& n, int l, int c, float4 (&pf)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = threadIdx.x + NT * u, kk = e & 15, jq = e >> 4;
    pf[u] = ldg4(pick(n.W, l) + (size_t) (KC * c + kk) * layer_ld(l, n.in0) + layer_hofs(l, n.in0) + 4 * jq);
  }
}
__device__ __forceinline__ void bwd_store(float* bs, const float4 (&pf)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = threadIdx.x + NT * u, kk = e & 15, j = 4 * (e >> 4);
    bs[(j + 0) * BP + kk] = pf[u].x;
    bs[(j + 1) * BP + kk] = pf[u].y;
    bs[(j + 2) * BP + kk] = pf[u].z;
    bs[(j + 3) * BP + kk] = pf[u].w;
  }
}

__global__ void __launch_bounds__(NT) sp_rows_backward_rows_kernel(int P, NetPtrs n, const float* __restrict__ g_raw, SavedView sv,
    WorkView wk) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_gz = lds + L_H;
  float* s_b  = lds + L_B;
  float* s_gh = lds + L_GH;
  float* s_hw = lds + L_HW;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int rt = wave & 1, cg = wave >> 1;
  const size_t r0 = (size_t) blockIdx.x * BM, Pp = pad_rows(P);
  float4 pf[2];
  bwd_load(n, NL - 1, 0, pf);
  // ---- head cotangents (zero beyond nout and P) and the heads' weights
#pragma unroll
  for (int u = 0; u < BM * 16 / NT; ++u) {
    const int e = tid + NT * u, row = e >> 4, c = e & 15;
    const float v = (c < n.nout && r0 + row < (size_t) P) ? g_raw[(r0 + row) * n.nout + c] : 0.f;
    s_gh[e] = v;
    wk.GH[(r0 + row) * 16 + c] = v;
  }
  for (int e = tid; e < 16 * W_; e += NT) {
    const int c = e >> 8, k = e & (W_ - 1);
    float v = 0.f;
    if (c < n.nout) {
      int hr;
      const int hd = head_of(c, hr);
      v = pick(n.head_w, hd)[(size_t) hr * W_ + k];
    }
    s_hw[e] = v;
  }
  bwd_store(s_b, pf);
  __syncthreads();
  {  // gZ_7 = (gH W_heads) * (Y_7 > 0): thread (feature j, rows 32 (tid >> 8) ..)
    const int j = tid & (W_ - 1), rb = 32 * (tid >> 8);
    float w[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) w[c] = s_hw[c * W_ + j];
    const float* y7 = sv.Y + ((size_t) (NL - 1) * Pp + r0) * W_ + j;
    float* gz7      = wk.GZ + ((size_t) (NL - 1) * Pp + r0) * W_ + j;
#pragma unroll 4
    for (int r = rb; r < rb + 32; ++r) {
      const float y = y7[(size_t) r * W_];
      float g = 0.f;
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        const float4 gh = *reinterpret_cast<const float4*>(s_gh + r * 16 + 4 * c4);
        g += gh.x * w[4 * c4] + gh.y * w[4 * c4 + 1] + gh.z * w[4 * c4 + 2] + gh.w * w[4 * c4 + 3];
      }
      g = y > 0.f ? g : 0.f;
      s_gz[r * HP + j]      = g;
      gz7[(size_t) r * W_] = g;
    }
  }
  __syncthreads();
  // ---- gY_{l-1} = gZ_l W_l[:, hidden], l = 7 .. 1: 112 chunks of 16 output rows
  int buf = 0, nl = NL - 1, nc = 1;
  f32x16 acc[2];
#pragma unroll 1
  for (int l = NL - 1; l >= 1; --l) {
    float y[2][16];  // Y_{l-1} at this lane's accumulator positions (requested before the stream: consumed at its end)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q)
        y[c][q] = sv.Y[((size_t) (l - 1) * Pp + r0 + 32 * rt + acc_row(q, h)) * W_ + 64 * cg + 32 * c + i];
    zero16(acc[0]), zero16(acc[1]);
#pragma unroll 1
    for (int c = 0; c < W_ / KC; ++c) {
      const bool more = nl >= 1;
      if (more) bwd_load(n, nl, nc, pf);
      mma_rows<KC, BP>(acc, s_gz + (32 * rt + i) * HP + KC * c + 4 * h, s_b + buf * W_ * BP + (64 * cg + i) * BP + 4 * h);
      if (more) {
        bwd_store(s_b + (buf ^ 1) * W_ * BP, pf);
        if (++nc == W_ / KC) nc = 0, --nl;
      }
      __syncthreads();
      buf ^= 1;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int o = 64 * cg + 32 * c + i;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 32 * rt + acc_row(q, h);
        const float g = y[c][q] > 0.f ? acc[c][q] : 0.f;
        s_gz[row * HP + o] = g;
        wk.GZ[((size_t) (l - 1) * Pp + r0 + row) * W_ + o] = g;
      }
    }
    __syncthreads();
  }
}

// =================================================================================================== backward, launch B
// tile t: [0,4) layer 0 over x0 (outputs 64 t ..); [4,116) layer 1 + (t - 4) / 16 over Y_{l-1}, outputs 64 (tt / 4), inputs
// 64 (tt % 4); [116,120) layer 5's input part over x0; [120,124) the heads (16 output rows, nout used) over Y_7, inputs 64 (t - 120)
struct TileInfo {
  int layer, o0, k0, lda, ldx, bias_row;  // bias_row: row of GBP this tile's column sums go to, or -1
  const float* A;
  const float* X;
};
__device__ __forceinline__ TileInfo tile_info(int t, int P, const SavedView& sv, const WorkView& wk) {
  const size_t Pp = pad_rows(P);
  TileInfo ti;
  ti.lda = W_;
  if (t < 4) {
    ti.layer = 0, ti.o0 = 64 * t, ti.k0 = 0, ti.X = sv.x0, ti.ldx = XC, ti.bias_row = 0;
  } else if (t < 116) {
    const int tt = (t - 4) % 16;
    ti.layer = 1 + (t - 4) / 16, ti.o0 = 64 * (tt / 4), ti.k0 = 64 * (tt % 4);
    ti.X = sv.Y + (size_t) (ti.layer - 1) * Pp * W_, ti.ldx = W_, ti.bias_row = tt % 4 == 0 ? ti.layer : -1;
  } else if (t < 120) {
    ti.layer = SKIP + 1, ti.o0 = 64 * (t - 116), ti.k0 = 0, ti.X = sv.x0, ti.ldx = XC, ti.bias_row = -1;
  } else {
    ti.layer = NL, ti.o0 = 0, ti.k0 = 64 * (t - 120), ti.X = sv.Y + (size_t) (NL - 1) * Pp * W_, ti.ldx = W_;
    ti.bias_row = t == 120 ? NL : -1;
  }
  if (ti.layer < NL) ti.A = wk.GZ + (size_t) ti.layer * Pp * W_;
  else ti.A = wk.GH, ti.lda = 16;
  return ti;
}

__global__ void __launch_bounds__(256) sp_rows_backward_weights_kernel(int P, SavedView sv, WorkView wk) {
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const int S = n_splits(P), job = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (job >= S * NTILE) return;
  const int split = job / NTILE, t = job - split * NTILE;
  const TileInfo ti = tile_info(t, P, sv, wk);
  const int rps = split_rows(P);
  const int Pp = (int) pad_rows(P), rb = min(split * rps, Pp), re = min(rb + rps, Pp);
  // lane (i, h): A columns o0 + 2 i, + 1 (tiles a = 0, 1) and X columns k0 + 2 i, + 1 (tiles c = 0, 1) of row r + h
  const bool avalid = ti.layer < NL || 2 * i < 16;
  const float* ap = ti.A + (size_t) h * ti.lda + (avalid ? ti.o0 + 2 * i : 0);
  const float* xp = ti.X + (size_t) h * ti.ldx + ti.k0 + 2 * i;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) zero16(acc[a][c]);
  float2 cs = make_float2(0.f, 0.f);
  constexpr int BATCH = 8;  // 2-row steps per batch (rb, re are multiples of 16)
  float2 av[2][BATCH], xv[2][BATCH];
  auto fetch = [&](int r, float2 (&a)[BATCH], float2 (&x)[BATCH]) {
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      a[u] = *reinterpret_cast<const float2*>(ap + (size_t) (r + 2 * u) * ti.lda);
      x[u] = *reinterpret_cast<const float2*>(xp + (size_t) (r + 2 * u) * ti.ldx);
      if (!avalid) a[u] = make_float2(0.f, 0.f);
    }
  };
  auto consume = [&](const float2 (&a)[BATCH], const float2 (&x)[BATCH]) {
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      cs.x += a[u].x, cs.y += a[u].y;
      acc[0][0] = mfma32(a[u].x, x[u].x, acc[0][0]);
      acc[0][1] = mfma32(a[u].x, x[u].y, acc[0][1]);
      acc[1][0] = mfma32(a[u].y, x[u].x, acc[1][0]);
      acc[1][1] = mfma32(a[u].y, x[u].y, acc[1][1]);
    }
  };
  if (rb < re) {
    fetch(rb, av[0], xv[0]);
    for (int r = rb; r < re; r += 4 * BATCH) {
      if (r + 2 * BATCH < re) fetch(r + 2 * BATCH, av[1], xv[1]);
      __builtin_amdgcn_sched_barrier(0);
      consume(av[0], xv[0]);
      if (r + 2 * BATCH < re) {
        if (r + 4 * BATCH < re) fetch(r + 4 * BATCH, av[0], xv[0]);
        __builtin_amdgcn_sched_barrier(0);
        consume(av[1], xv[1]);
      }
    }
  }
  // partial tile [o local][k local]: register q of acc[a][c] in lane (i, h) <-> o = 2 acc_row(q, h) + a, k = 2 i + c
  float* part = wk.PART + (size_t) job * 4096;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 16; ++q)
      *reinterpret_cast<float2*>(part + (2 * acc_row(q, h) + a) * 64 + 2 * i) = make_float2(acc[a][0][q], acc[a][1][q]);
  if (ti.bias_row >= 0) {
    cs.x += __shfl_xor(cs.x, 32), cs.y += __shfl_xor(cs.y, 32);
    if (h == 0) *reinterpret_cast<float2*>(wk.GBP + ((size_t) split * NBIAS + ti.bias_row) * W_ + ti.o0 + 2 * i) = cs;
  }
}

// =================================================================================================== backward, launch C
// sum over the S splits in split order, 16 loads in flight per round (one load -> add chain was S dependent round trips)
__device__ __forceinline__ float split_sum(const float* p, size_t stride, int S) {
  float v = 0.f;
  for (int s0 = 0; s0 < S; s0 += 16) {
    float t[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) t[u] = p[(size_t) min(s0 + u, S - 1) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (s0 + u < S) v += t[u];
  }
  return v;
}
__device__ __forceinline__ float bias_sum(const WorkView& wk, int S, int row, int o) {
  return split_sum(wk.GBP + (size_t) row * W_ + o, (size_t) NBIAS * W_, S);
}

// the time columns of layers 0 and 5 and the time network (one workgroup of 256 threads: thread o = feature o)
__device__ __forceinline__ void time_backward(int P, const NetPtrs& n, const GradPtrs& g, const SavedView& sv, const WorkView& wk, float* s_buf) {
  const int tid = threadIdx.x, S = n_splits(P);
  float* s_prod = s_buf;              // [TOUT][256]
  float* s_gt   = s_buf + TOUT * W_;  // [32]
  const float gb0 = bias_sum(wk, S, 0, tid), gb5 = bias_sum(wk, S, SKIP + 1, tid);
  const size_t ld0 = layer_ld(0, n.in0), ld5 = layer_ld(SKIP + 1, n.in0);
  for (int c = 0; c < n.tw; ++c) {  // gW_l[:, 63 + c] = gb_l t_emb[c]
    g.W[0][tid * ld0 + PDIM + c]        = gb0 * sv.temb[c];
    g.W[SKIP + 1][tid * ld5 + PDIM + c] = gb5 * sv.temb[c];
  }
  if (!n.tw1) return;  // raw time encoding: the time is data, nothing more to do
  const float* w0 = n.W[0] + tid * ld0 + PDIM;
  const float* w5 = n.W[SKIP + 1] + tid * ld5 + PDIM;
  float pr[TOUT];
#pragma unroll
  for (int c = 0; c < TOUT; ++c) pr[c] = gb0 * w0[c] + gb5 * w5[c];
#pragma unroll
  for (int c = 0; c < TOUT; ++c) s_prod[c * W_ + tid] = pr[c];
  __syncthreads();
  if (tid < TOUT * 8) {
    const int c = tid >> 3, part = tid & 7;
    float v = 0.f;
    for (int o = part; o < W_; o += 8) v += s_prod[c * W_ + o];
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    if (part == 0) s_gt[c] = v;
  }
  __syncthreads();
  // second linear: gW2 [30][256] = g_t (x) hid, gb2 = g_t;  g_hid = W2^T g_t * (hid > 0);  first: gW1 = g_hid (x) freq(t), gb1 = g_hid
  const float hid = sv.thid[tid];
  float gh = 0.f;
#pragma unroll
  for (int c = 0; c < TOUT; ++c) {
    g.tw2[c * THID + tid] = s_gt[c] * hid;
    gh += s_gt[c] * n.tw2[c * THID + tid];
  }
  gh = hid > 0.f ? gh : 0.f;
  if (tid < TOUT) g.tb2[tid] = s_gt[tid];
  g.tb1[tid] = gh;
#pragma unroll
  for (int k = 0; k < TDIM; ++k) g.tw1[tid * TDIM + k] = gh * sv.tenc[k];
}

constexpr int REDUCE_GROUPS = NTILE * 4096 / 256;
__global__ void __launch_bounds__(256) sp_rows_backward_reduce_kernel(int P, NetPtrs n, GradPtrs g, SavedView sv, WorkView wk) {
  __shared__ float s_buf[TOUT * W_ + 32];
  const int S = n_splits(P), tid = threadIdx.x;
  if ((int) blockIdx.x == REDUCE_GROUPS) {  // bias gradients
    for (int row = 0; row < NBIAS; ++row) {
      const float v = bias_sum(wk, S, row, tid);
      if (row < NL) {
        g.b[row][tid] = v;
      } else if (tid < n.nout) {
        int hr;
        const int hd = head_of(tid, hr);
        pick(g.head_b, hd)[hr] = v;
      }
    }
    return;
  }
  if ((int) blockIdx.x == REDUCE_GROUPS + 1) {
    time_backward(P, n, g, sv, wk, s_buf);
    return;
  }
  const int e = blockIdx.x * 256 + tid, t = e >> 12, ol = (e >> 6) & 63, kl = e & 63;
  const float v = split_sum(wk.PART + (size_t) e, (size_t) NTILE * 4096, S);
  const TileInfo ti = tile_info(t, P, sv, wk);
  const int o = ti.o0 + ol, k = ti.k0 + kl;
  if (ti.layer == NL) {
    if (o < n.nout) {
      int hr;
      const int hd = head_of(o, hr);
      pick(g.head_w, hd)[(size_t) hr * W_ + k] = v;
    }
  } else if (ti.X == sv.x0) {  // the x_emb columns of layer 0 / 5 (column 63 of x0 is the zero pad)
    if (k < PDIM) g.W[ti.layer][(size_t) o * layer_ld(ti.layer, n.in0) + k] = v;
  } else {
    g.W[ti.layer][(size_t) o * layer_ld(ti.layer, n.in0) + layer_hofs(ti.layer, n.in0) + k] = v;
  }
}

NetPtrs net_ptrs(const skgs_sp_net* d) {
  NetPtrs n;
  n.points = d->points, n.time = d->time;
  n.tw1 = d->time_w1, n.tb1 = d->time_b1, n.tw2 = d->time_w2, n.tb2 = d->time_b2;
  for (int l = 0; l < NL; ++l) n.W[l] = d->W[l], n.b[l] = d->b[l];
  n.head_w[0] = d->warp_w, n.head_b[0] = d->warp_b;
  n.head_w[1] = d->rotation_w, n.head_b[1] = d->rotation_b;
  n.head_w[2] = d->scaling_w, n.head_b[2] = d->scaling_b;
  n.head_w[3] = d->local_w, n.head_b[3] = d->local_b;
  n.nout = (d->local_w && d->local_b) ? NOUT_MAX : 10;
  if (d->flags & SKGS_SP_NET_RAW_TIME) {
    n.tdim = 1 + 2 * ((d->flags >> 8) & 0xff);
    n.tw = n.tdim;
    n.tw1 = n.tb1 = n.tw2 = n.tb2 = nullptr;
  } else {
    n.tdim = TDIM, n.tw = TOUT;
  }
  n.in0 = PDIM + n.tw;
  return n;
}
bool net_complete(const skgs_sp_net* d) {
  bool ok = d->warp_w && d->warp_b && d->scaling_w && d->scaling_b && d->rotation_w && d->rotation_b;
  if (d->flags & SKGS_SP_NET_RAW_TIME) ok = ok && ((d->flags >> 8) & 0xff) <= 15;
  else ok = ok && d->time_w1 && d->time_b1 && d->time_w2 && d->time_b2;
  for (int l = 0; l < NL; ++l) ok = ok && d->W[l] && d->b[l];
  return ok;
}
bool flags_known(int32_t f) { return (f & ~(SKGS_SP_NET_RAW_TIME_FLAG | (0xff << 8))) == 0; }
int allow_rows_lds() {
  static int rc = [] {
    bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(sp_rows_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                  (int) ROWS_LDS_BYTES) == hipSuccess;
    ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(sp_rows_backward_rows_kernel),
                   hipFuncAttributeMaxDynamicSharedMemorySize, (int) ROWS_LDS_BYTES) == hipSuccess;
    return ok ? 0 : 1;
  }();
  return rc;
}

}  // namespace
}  // namespace skgs

using namespace skgs;

extern "C" {

size_t skgs_sp_net_rows_saved_bytes(int32_t P) { return P > 0 ? saved_floats(P) * 4 : 0; }
size_t skgs_sp_net_rows_workspace_bytes(int32_t P) { return P > 0 ? work_floats(P) * 4 : 0; }

int skgs_sp_net_rows_forward(const skgs_sp_net* net, float* raw, void* saved, size_t saved_bytes, skgs_stream_t stream) {
  SKGS_REQUIRE(net && net->M >= 1, "sp_net_rows_forward: NULL descriptor or P < 1");
  SKGS_REQUIRE(!(net->flags & SKGS_SP_NET_LBS_C) && flags_known(net->flags),
      "sp_net_rows_forward: flags other than SKGS_SP_NET_RAW_TIME_DEGREE (LBS_c is the sp stage's epilogue)");
  SKGS_REQUIRE(net->points && net->time && net_complete(net), "sp_net_rows_forward: NULL points / time / parameter");
  SKGS_REQUIRE(raw, "sp_net_rows_forward: no output");
  SKGS_REQUIRE(!saved || saved_bytes >= skgs_sp_net_rows_saved_bytes(net->M), "sp_net_rows_forward: saved buffer too small");
  SKGS_REQUIRE(allow_rows_lds() == 0, "sp_net_rows_forward: cannot raise the dynamic LDS limit");
  hipStream_t s    = (hipStream_t) stream;
  const NetPtrs n  = net_ptrs(net);
  const SavedView sv = saved ? saved_view(saved, net->M) : SavedView{};
  hipLaunchKernelGGL(sp_rows_forward_kernel, dim3((unsigned) (pad_rows(net->M) / BM)), dim3(NT), ROWS_LDS_BYTES, s, net->M, n, raw, sv,
      saved ? 1 : 0);
  SKGS_CHECK_HIP(hipGetLastError());
  return 0;
}

int skgs_sp_net_rows_backward(const skgs_sp_net* net, const skgs_sp_net* grads, const float* g_raw, const void* saved,
    size_t saved_bytes, void* workspace, size_t workspace_bytes, skgs_stream_t stream) {
  SKGS_REQUIRE(net && grads && net->M >= 1, "sp_net_rows_backward: NULL descriptor or P < 1");
  SKGS_REQUIRE(!(net->flags & SKGS_SP_NET_LBS_C) && flags_known(net->flags),
      "sp_net_rows_backward: flags other than SKGS_SP_NET_RAW_TIME_DEGREE (LBS_c is the sp stage's epilogue)");
  SKGS_REQUIRE(net_complete(net), "sp_net_rows_backward: NULL parameter");
  SKGS_REQUIRE(g_raw, "sp_net_rows_backward: no cotangent");
  SKGS_REQUIRE(saved && saved_bytes >= skgs_sp_net_rows_saved_bytes(net->M), "sp_net_rows_backward: saved buffer too small");
  SKGS_REQUIRE(workspace && workspace_bytes >= skgs_sp_net_rows_workspace_bytes(net->M), "sp_net_rows_backward: workspace too small");
  const int P = net->M;
  const NetPtrs n = net_ptrs(net);
  GradPtrs g;
  g.tw1 = const_cast<float*>(grads->time_w1), g.tb1 = const_cast<float*>(grads->time_b1);
  g.tw2 = const_cast<float*>(grads->time_w2), g.tb2 = const_cast<float*>(grads->time_b2);
  bool ok = true;
  for (int l = 0; l < NL; ++l) {
    g.W[l] = const_cast<float*>(grads->W[l]), g.b[l] = const_cast<float*>(grads->b[l]);
    ok = ok && g.W[l] && g.b[l];
  }
  g.head_w[0] = const_cast<float*>(grads->warp_w), g.head_b[0] = const_cast<float*>(grads->warp_b);
  g.head_w[1] = const_cast<float*>(grads->rotation_w), g.head_b[1] = const_cast<float*>(grads->rotation_b);
  g.head_w[2] = const_cast<float*>(grads->scaling_w), g.head_b[2] = const_cast<float*>(grads->scaling_b);
  g.head_w[3] = const_cast<float*>(grads->local_w), g.head_b[3] = const_cast<float*>(grads->local_b);
  for (int k = 0; k < (n.nout == NOUT_MAX ? 4 : 3); ++k) ok = ok && g.head_w[k] && g.head_b[k];
  if (n.tw1) ok = ok && g.tw1 && g.tb1 && g.tw2 && g.tb2;
  SKGS_REQUIRE(ok, "sp_net_rows_backward: NULL gradient pointer");
  SKGS_REQUIRE(allow_rows_lds() == 0, "sp_net_rows_backward: cannot raise the dynamic LDS limit");
  hipStream_t s      = (hipStream_t) stream;
  const SavedView sv = saved_view(const_cast<void*>(saved), P);
  const WorkView wk  = work_view(workspace, P);
  hipLaunchKernelGGL(sp_rows_backward_rows_kernel, dim3((unsigned) (pad_rows(P) / BM)), dim3(NT), ROWS_LDS_BYTES, s, P, n, g_raw, sv, wk);
  SKGS_CHECK_HIP(hipGetLastError());
  const int jobs = n_splits(P) * NTILE;
  hipLaunchKernelGGL(sp_rows_backward_weights_kernel, dim3((jobs + 3) / 4), dim3(256), 0, s, P, sv, wk);
  SKGS_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sp_rows_backward_reduce_kernel, dim3(REDUCE_GROUPS + 2), dim3(256), 0, s, P, n, g, sv, wk);
  SKGS_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
