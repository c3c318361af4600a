// joint_loss.hip -- the joint-discovery loss of stage sp (networks/sk_gs.py:1309-1336, `joint` / `joint_all` in exps/default.yaml:93-94),
// run in every stage-sp iteration from step 20 000 on.  Per ordered pair (a, b) of the M superpoints, with R_a, t_a = quaternion_to_Rt of
// spT[a] (the polynomial of my_ext/ops_3d/rigid.py:110-130 on the UNNORMALISED quaternion) and p_ab = joint_pos[a, b]:
//
//   d1[a,b] = | R_b p_ab + t_b - R_a p_ab - t_a |                          canonical_time_id >= 0
//           = | R_b^-1 (R_a p_ab + t_a - t_b) - p_ab |                      canonical_time_id <  0   (inverse(T_b) @ T_a applied to p_ab)
//   d2[a,b] = | R_b p_ab + t_b - R_a p_ba - t_a |                           (symmetric in a, b)
//   jd = d1 + d2;   all = mean(jd);   best = mean over the tree's edges (a, parent a) of (jd[a, p] + jd[p, a]) / 2
//
// torch builds two [M, M, 4, 4] broadcast products for it (16 MB each at M = 512) and ~60 launches forward, ~40 backward.  Here:
//   forward  -- one launch over 16 x 16 tiles of pairs: jd, the EMA of joint_cost (training) and fixed-order partial sums of jd;
//               a one-workgroup launch then reduces `all` and the edge terms of `best` (after the caller's tree update, if any);
//   backward -- one launch over the same tiles: the gradient of joint_pos gathered per element without atomics, per-tile row / column
//               partial sums of dL/d(R, t) (and dL/dR^-1 for the inverse branch); a finalize launch per node sums them in a fixed order,
//               applies the inverse's chain and the Jacobian of the quaternion polynomial.
// No float atomics: both directions are bitwise reproducible.  A pair (a, a) is exactly zero in exact arithmetic: it contributes 0 and no
// gradient (torch's norm backward gives none to a zero vector; its own diagonal is rounding noise).
#include <algorithm>

#include "skgs_common.h"

namespace skgs {
namespace {

constexpr int JT         = 16;        // tile edge: a workgroup owns pairs (A0 .. A0+15) x (B0 .. B0+15)
constexpr int JL_THREADS = JT * JT;   // thread (ty, tx) = pair (A0 + ty, B0 + tx); a wave holds four tile rows
constexpr int JL_MAX_M   = 1024;
constexpr int NODE_F     = 22;        // per node in LDS: R (9), t (3), R^-1 (9), padding
constexpr int ROW_F      = 12;        // row partials per node: dL/dR (9), dL/dt (3)
constexpr int COL_F      = 21;        // column partials per node: dL/dR, dL/dt, dL/dR^-1

inline int jl_tiles(int M) { return (M + JT - 1) / JT; }

// R(q) of quaternion_to_Rt, q = (x, y, z, w), in the reference's operation order
__device__ __forceinline__ void quat_R(float x, float y, float z, float w, float* R) {
  R[0] = 1.f - 2.f * y * y - 2.f * z * z;
  R[1] = 2.f * x * y - 2.f * w * z;
  R[2] = 2.f * w * y + 2.f * x * z;
  R[3] = 2.f * x * y + 2.f * w * z;
  R[4] = 1.f - 2.f * x * x - 2.f * z * z;
  R[5] = 2.f * y * z - 2.f * w * x;
  R[6] = 2.f * x * z - 2.f * w * y;
  R[7] = 2.f * w * x + 2.f * y * z;
  R[8] = 1.f - 2.f * x * x - 2.f * y * y;
}

// the general 3x3 inverse (adjugate / determinant, in double): R is not a rotation for an unnormalised q
__device__ __forceinline__ void inv3(const float* R, double* I) {
  const double a = R[0], b = R[1], c = R[2], d = R[3], e = R[4], f = R[5], g = R[6], h = R[7], k = R[8];
  const double A = e * k - f * h, B = f * g - d * k, Cc = d * h - e * g;
  const double det = a * A + b * B + c * Cc;
  const double r   = 1.0 / det;
  I[0] = A * r;  I[1] = (c * h - b * k) * r;  I[2] = (b * f - c * e) * r;
  I[3] = B * r;  I[4] = (a * k - c * g) * r;  I[5] = (c * d - a * f) * r;
  I[6] = Cc * r; I[7] = (b * g - a * h) * r;  I[8] = (a * e - b * d) * r;
}

// node n's R, t, R^-1 into LDS (zeros past M)
__device__ __forceinline__ void load_node(int M, int n, const float* __restrict__ spT, float* s) {
  if (n >= M) {
    for (int k = 0; k < NODE_F; ++k) s[k] = 0.f;
    return;
  }
  const float* q = spT + (size_t) n * 7;
  quat_R(q[3], q[4], q[5], q[6], s);
  s[9] = q[0], s[10] = q[1], s[11] = q[2];
  double I[9];
  inv3(s, I);
  for (int k = 0; k < 9; ++k) s[12 + k] = (float) I[k];
  s[21] = 0.f;
}

__device__ __forceinline__ void mat_vec(const float* R, const float* p, float* o) {
  o[0] = R[0] * p[0] + R[1] * p[1] + R[2] * p[2];
  o[1] = R[3] * p[0] + R[4] * p[1] + R[5] * p[2];
  o[2] = R[6] * p[0] + R[7] * p[1] + R[8] * p[2];
}

__device__ __forceinline__ void mat_t_vec(const float* R, const float* g, float* o) {   // R^T g
  o[0] = R[0] * g[0] + R[3] * g[1] + R[6] * g[2];
  o[1] = R[1] * g[0] + R[4] * g[1] + R[7] * g[2];
  o[2] = R[2] * g[0] + R[5] * g[1] + R[8] * g[2];
}

__device__ __forceinline__ float norm3(const float* v) { return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// p_ab (tile rows a, columns b) and p_ba (tile rows b, columns a) with coalesced loads; rows padded to 49 floats
__device__ __forceinline__ void load_pair_tiles(int M, int A0, int B0, const float* __restrict__ jp, float (*s_pab)[JT * 3 + 1],
    float (*s_pba)[JT * 3 + 1]) {
  for (int e = threadIdx.x; e < JT * JT * 3; e += JL_THREADS) {
    const int r = e / (JT * 3), c = e % (JT * 3);
    const int ra = A0 + r, cb = B0 + c / 3, rb = B0 + r, ca = A0 + c / 3;
    s_pab[r][c] = (ra < M && cb < M) ? jp[((size_t) ra * M + B0) * 3 + c] : 0.f;
    s_pba[r][c] = (rb < M && ca < M) ? jp[((size_t) rb * M + A0) * 3 + c] : 0.f;
  }
}

template <bool INV>
__device__ __forceinline__ void pair_vectors(const float* na, const float* nb, const float* pab, const float* pba, float* u, float* v, float* w) {
  float Rbp[3], Rap[3], Rapba[3];
  mat_vec(nb, pab, Rbp);
  mat_vec(na, pab, Rap);
  if (INV) {       // w = R_a p + t_a - t_b ; u = R_b^-1 w - p
    for (int k = 0; k < 3; ++k) w[k] = (Rap[k] + na[9 + k]) - nb[9 + k];
    float Bw[3];
    mat_vec(nb + 12, w, Bw);
    for (int k = 0; k < 3; ++k) u[k] = Bw[k] - pab[k];
  } else {
    for (int k = 0; k < 3; ++k) u[k] = ((Rbp[k] + nb[9 + k]) - Rap[k]) - na[9 + k];
  }
  mat_vec(na, pba, Rapba);
  for (int k = 0; k < 3; ++k) v[k] = (Rbp[k] + nb[9 + k]) - (Rapba[k] + na[9 + k]);
}

template <bool INV>
__global__ void __launch_bounds__(JL_THREADS) joint_loss_forward_kernel(int M, const float* __restrict__ spT, const float* __restrict__ jp,
    const float* __restrict__ cost_in, float momentum, float one_minus_momentum, float* __restrict__ cost_out, float* __restrict__ jd,
    float* __restrict__ partials) {
  __shared__ float s_pab[JT][JT * 3 + 1], s_pba[JT][JT * 3 + 1];
  __shared__ float s_na[JT][NODE_F], s_nb[JT][NODE_F];
  __shared__ float s_red[4];
  const int A0 = blockIdx.y * JT, B0 = blockIdx.x * JT;
  const int tx = threadIdx.x % JT, ty = threadIdx.x / JT;
  load_pair_tiles(M, A0, B0, jp, s_pab, s_pba);
  if (threadIdx.x < JT) load_node(M, A0 + threadIdx.x, spT, s_na[threadIdx.x]);
  else if (threadIdx.x < 2 * JT) load_node(M, B0 + threadIdx.x - JT, spT, s_nb[threadIdx.x - JT]);
  __syncthreads();
  const int a = A0 + ty, b = B0 + tx;
  float d = 0.f;
  if (a < M && b < M) {
    if (a != b) {
      float u[3], v[3], w[3];
      pair_vectors<INV>(s_na[ty], s_nb[tx], &s_pab[ty][tx * 3], &s_pba[tx][ty * 3], u, v, w);
      d = norm3(u) + norm3(v);
    }
    const size_t i = (size_t) a * M + b;
    jd[i] = d;
    if (cost_out) cost_out[i] = cost_in[i] * momentum + d * one_minus_momentum;
  }
  // fixed order: lanes of a wave by xor shuffles, then the four waves in index order
  float s = d;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// one workgroup: out[0] = best (mean over the edges a -> parent[a] of (jd[a,p] + jd[p,a]) / 2), out[1] = all (mean of jd)
__global__ void __launch_bounds__(256) joint_loss_reduce_kernel(int M, int edges, int n_partials, const int32_t* __restrict__ parent,
    const float* __restrict__ jd, const float* __restrict__ partials, float* __restrict__ out) {
  __shared__ double s_a[256], s_b[256];
  double sa = 0.0, sb = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += 256) sa += (double) partials[i];
  for (int a = threadIdx.x; a < M; a += 256) {
    const int p = parent[a];
    if (p >= 0) sb += 0.5 * ((double) jd[(size_t) a * M + p] + (double) jd[(size_t) p * M + a]);
  }
  s_a[threadIdx.x] = sa, s_b[threadIdx.x] = sb;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int) threadIdx.x < h) s_a[threadIdx.x] += s_a[threadIdx.x + h], s_b[threadIdx.x] += s_b[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float) (s_b[0] / (double) edges);
    out[1] = (float) (s_a[0] / ((double) M * (double) M));
  }
}

// the loss's weight on jd[a, b]: all / M^2 + best's share when (a, b) or (b, a) is an edge
__device__ __forceinline__ float pair_weight(int a, int b, const int32_t* __restrict__ parent, float g_all_mm, float g_best_e) {
  return g_all_mm + g_best_e * (float) ((parent[a] == b) + (parent[b] == a));
}

template <bool INV, bool NODES>
__global__ void __launch_bounds__(JL_THREADS) joint_loss_backward_kernel(int M, int edges, const float* __restrict__ spT,
    const float* __restrict__ jp, const int32_t* __restrict__ parent, const float* __restrict__ grad_best, const float* __restrict__ grad_all,
    float* __restrict__ g_jp, float* __restrict__ row_part, float* __restrict__ col_part) {
  __shared__ float s_pab[JT][JT * 3 + 1], s_pba[JT][JT * 3 + 1];
  __shared__ float s_na[JT][NODE_F], s_nb[JT][NODE_F];
  __shared__ float s_col[4][JT][COL_F];
  const int A0 = blockIdx.y * JT, B0 = blockIdx.x * JT;
  const int tx = threadIdx.x % JT, ty = threadIdx.x / JT;
  load_pair_tiles(M, A0, B0, jp, s_pab, s_pba);
  if (threadIdx.x < JT) load_node(M, A0 + threadIdx.x, spT, s_na[threadIdx.x]);
  else if (threadIdx.x < 2 * JT) load_node(M, B0 + threadIdx.x - JT, spT, s_nb[threadIdx.x - JT]);
  __syncthreads();
  const float g_all_mm = grad_all ? *grad_all / ((float) M * (float) M) : 0.f;
  const float g_best_e = grad_best ? *grad_best * (0.5f / (float) edges) : 0.f;
  const int a = A0 + ty, b = B0 + tx;
  float ra[ROW_F], cb[COL_F];    // this pair's dL/d(R_a, t_a) and dL/d(R_b, t_b, R_b^-1)
#pragma unroll
  for (int k = 0; k < ROW_F; ++k) ra[k] = 0.f;
#pragma unroll
  for (int k = 0; k < COL_F; ++k) cb[k] = 0.f;
  if (a < M && b < M) {
    float gp[3] = {0.f, 0.f, 0.f};
    if (a != b) {
      const float* na = s_na[ty];
      const float* nb = s_nb[tx];
      const float* pab = &s_pab[ty][tx * 3];
      const float* pba = &s_pba[tx][ty * 3];
      float u[3], v[3], w[3];
      pair_vectors<INV>(na, nb, pab, pba, u, v, w);
      const float c_ab = pair_weight(a, b, parent, g_all_mm, g_best_e);
      const float c_ba = pair_weight(b, a, parent, g_all_mm, g_best_e);
      const float nu = norm3(u), nv = norm3(v);
      float g1[3] = {0.f, 0.f, 0.f}, g2[3] = {0.f, 0.f, 0.f}, g2s[3] = {0.f, 0.f, 0.f};
      if (nu > 0.f)
        for (int k = 0; k < 3; ++k) g1[k] = c_ab * (u[k] / nu);
      if (nv > 0.f)
        for (int k = 0; k < 3; ++k) g2[k] = c_ab * (v[k] / nv), g2s[k] = (c_ab + c_ba) * (v[k] / nv);
      // d1
      float t0[3], t1[3];
      if (INV) {        // u = B w - p, w = R_a p + t_a - t_b:  h = B^T g1;  dp = R_a^T h - g1;  dR_a = h p^T, dt_a = h, dt_b = -h, dB = g1 w^T
        float h[3];
        mat_t_vec(nb + 12, g1, h);
        mat_t_vec(na, h, t0);
        for (int k = 0; k < 3; ++k) gp[k] += t0[k] - g1[k];
        if (NODES) {
          for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) ra[i * 3 + j] += h[i] * pab[j], cb[12 + i * 3 + j] += g1[i] * w[j];
            ra[9 + i] += h[i], cb[9 + i] -= h[i];
          }
        }
      } else {          // u = (R_b - R_a) p + t_b - t_a
        mat_t_vec(nb, g1, t0);
        mat_t_vec(na, g1, t1);
        for (int k = 0; k < 3; ++k) gp[k] += t0[k] - t1[k];
        if (NODES) {
          for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) ra[i * 3 + j] -= g1[i] * pab[j], cb[i * 3 + j] += g1[i] * pab[j];
            ra[9 + i] -= g1[i], cb[9 + i] += g1[i];
          }
        }
      }
      // d2[a,b] (weight c_ab) and d2[b,a] = |-v| (weight c_ba) both reach p_ab through R_b^T v / |v|; the nodes take d2[a,b] here, d2[b,a]
      // in the thread of pair (b, a)
      mat_t_vec(nb, g2s, t0);
      for (int k = 0; k < 3; ++k) gp[k] += t0[k];
      if (NODES) {
        for (int i = 0; i < 3; ++i) {
          for (int j = 0; j < 3; ++j) cb[i * 3 + j] += g2[i] * pab[j], ra[i * 3 + j] -= g2[i] * pba[j];
          cb[9 + i] += g2[i], ra[9 + i] -= g2[i];
        }
      }
    }
    float* o = g_jp + ((size_t) a * M + b) * 3;
    o[0] = gp[0], o[1] = gp[1], o[2] = gp[2];
  }
  if (!NODES) return;
  // row sums over tx (16 adjacent lanes), column sums over ty (lane groups of 16 in a wave, then the four waves) -- fixed order
#pragma unroll
  for (int k = 0; k < ROW_F; ++k) {
    float s = ra[k];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 8);
    ra[k] = s;
  }
  if (tx == 0 && a < M) {
    float* o = row_part + ((size_t) blockIdx.x * M + a) * ROW_F;
    for (int k = 0; k < ROW_F; ++k) o[k] = ra[k];
  }
#pragma unroll
  for (int k = 0; k < COL_F; ++k) {
    float s = cb[k];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    cb[k] = s;
  }
  if ((threadIdx.x & 63) < JT)
    for (int k = 0; k < COL_F; ++k) s_col[threadIdx.x >> 6][tx][k] = cb[k];
  __syncthreads();
  for (int e = threadIdx.x; e < JT * COL_F; e += JL_THREADS) {
    const int c = e / COL_F, k = e % COL_F;
    if (B0 + c < M)
      col_part[((size_t) blockIdx.y * M + B0 + c) * COL_F + k] = ((s_col[0][c][k] + s_col[1][c][k]) + s_col[2][c][k]) + s_col[3][c][k];
  }
}

// per node (one wave): the tiles' partial sums in index order, one lane per component; then the inverse's chain (dR += -R^-T dB R^-T)
// and the quaternion polynomial's Jacobian
template <bool INV>
__global__ void __launch_bounds__(64) joint_loss_finalize_kernel(int M, int tiles, const float* __restrict__ spT,
    const float* __restrict__ row_part, const float* __restrict__ col_part, float* __restrict__ g_spT) {
  __shared__ double s[ROW_F + COL_F];
  const int n = blockIdx.x, k = threadIdx.x;
  if (k < ROW_F) {
    double acc = 0.0;
    for (int t = 0; t < tiles; ++t) acc += row_part[((size_t) t * M + n) * ROW_F + k];
    s[k] = acc;
  } else if (k < ROW_F + COL_F) {
    double acc = 0.0;
    for (int t = 0; t < tiles; ++t) acc += col_part[((size_t) t * M + n) * COL_F + (k - ROW_F)];
    s[k] = acc;
  }
  __syncthreads();
  if (k != 0) return;
  double G[9], gt[3], dB[9];
  for (int i = 0; i < 9; ++i) G[i] = s[i] + s[ROW_F + i], dB[i] = s[ROW_F + 12 + i];
  for (int i = 0; i < 3; ++i) gt[i] = s[9 + i] + s[ROW_F + 9 + i];
  const float* q = spT + (size_t) n * 7;
  if (INV) {
    float R[9];
    double I[9], T[9];
    quat_R(q[3], q[4], q[5], q[6], R);
    inv3(R, I);
    // T = dB I^T ; G -= I^T T  (i.e. -I^T dB I^T)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) T[i * 3 + j] = dB[i * 3 + 0] * I[j * 3 + 0] + dB[i * 3 + 1] * I[j * 3 + 1] + dB[i * 3 + 2] * I[j * 3 + 2];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G[i * 3 + j] -= I[0 * 3 + i] * T[0 * 3 + j] + I[1 * 3 + i] * T[1 * 3 + j] + I[2 * 3 + i] * T[2 * 3 + j];
  }
  const double x = q[3], y = q[4], z = q[5], w = q[6];
  const double gx = 2.0 * (y * (G[1] + G[3]) + z * (G[2] + G[6]) + w * (G[7] - G[5])) - 4.0 * x * (G[4] + G[8]);
  const double gy = 2.0 * (x * (G[1] + G[3]) + z * (G[5] + G[7]) + w * (G[2] - G[6])) - 4.0 * y * (G[0] + G[8]);
  const double gz = 2.0 * (x * (G[2] + G[6]) + y * (G[5] + G[7]) + w * (G[3] - G[1])) - 4.0 * z * (G[0] + G[4]);
  const double gw = 2.0 * (y * (G[2] - G[6]) + z * (G[3] - G[1]) + x * (G[7] - G[5]));
  float* o = g_spT + (size_t) n * 7;
  o[0] = (float) gt[0], o[1] = (float) gt[1], o[2] = (float) gt[2];
  o[3] = (float) gx, o[4] = (float) gy, o[5] = (float) gz, o[6] = (float) gw;
}

}  // namespace
}  // namespace skgs

using namespace skgs;

extern "C" {

int32_t skgs_joint_loss_partials(int32_t M) { return M >= 1 ? jl_tiles(M) * jl_tiles(M) : 0; }

int skgs_joint_loss_forward(int32_t M, int32_t inverse_branch, const float* spT, const float* joint_pos, const float* cost_in, float momentum,
    float one_minus_momentum, float* cost_out, float* jd, float* partials, skgs_stream_t stream) {
  SKGS_REQUIRE(M >= 2 && M <= JL_MAX_M && spT && joint_pos && jd && partials, "joint_loss_forward: bad argument (2 <= M <= 1024)");
  SKGS_REQUIRE(cost_out == nullptr || cost_in != nullptr, "joint_loss_forward: the EMA needs the old joint_cost");
  hipStream_t s = (hipStream_t) stream;
  const int T  = jl_tiles(M);
  if (inverse_branch)
    hipLaunchKernelGGL(joint_loss_forward_kernel<true>, dim3(T, T), dim3(JL_THREADS), 0, s, M, spT, joint_pos, cost_in, momentum,
        one_minus_momentum, cost_out, jd, partials);
  else
    hipLaunchKernelGGL(joint_loss_forward_kernel<false>, dim3(T, T), dim3(JL_THREADS), 0, s, M, spT, joint_pos, cost_in, momentum,
        one_minus_momentum, cost_out, jd, partials);
  SKGS_CHECK_HIP(hipGetLastError());
  return 0;
}

int skgs_joint_loss_reduce(int32_t M, int32_t edges, const int32_t* parent, const float* jd, const float* partials, float* out,
    skgs_stream_t stream) {
  SKGS_REQUIRE(M >= 2 && M <= JL_MAX_M && edges >= 1 && parent && jd && partials && out, "joint_loss_reduce: bad argument");
  hipLaunchKernelGGL(joint_loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t) stream, M, edges, skgs_joint_loss_partials(M), parent, jd,
      partials, out);
  SKGS_CHECK_HIP(hipGetLastError());
  return 0;
}

size_t skgs_joint_loss_backward_workspace_bytes(int32_t M) {
  return M >= 1 ? (size_t) jl_tiles(M) * M * (ROW_F + COL_F) * sizeof(float) : 0;
}

int skgs_joint_loss_backward(int32_t M, int32_t inverse_branch, int32_t edges, const float* spT, const float* joint_pos, const int32_t* parent,
    const float* grad_best, const float* grad_all, float* g_joint_pos, float* g_spT, void* workspace, size_t workspace_bytes,
    skgs_stream_t stream) {
  SKGS_REQUIRE(M >= 2 && M <= JL_MAX_M && edges >= 1 && spT && joint_pos && parent && g_joint_pos, "joint_loss_backward: bad argument");
  SKGS_REQUIRE(g_spT == nullptr || (workspace && workspace_bytes >= skgs_joint_loss_backward_workspace_bytes(M)),
      "joint_loss_backward: workspace too small");
  hipStream_t s = (hipStream_t) stream;
  const int T    = jl_tiles(M);
  float* row     = g_spT ? (float*) workspace : nullptr;
  float* col     = g_spT ? row + (size_t) T * M * ROW_F : nullptr;
  const dim3 grid(T, T);
#define JL_BWD(INV, NODES)                                                                                                            \
  hipLaunchKernelGGL((joint_loss_backward_kernel<INV, NODES>), grid, dim3(JL_THREADS), 0, s, M, edges, spT, joint_pos, parent, grad_best, \
      grad_all, g_joint_pos, row, col)
  if (inverse_branch) {
    if (g_spT) JL_BWD(true, true);
    else JL_BWD(true, false);
  } else {
    if (g_spT) JL_BWD(false, true);
    else JL_BWD(false, false);
  }
#undef JL_BWD
  if (g_spT) {
    if (inverse_branch)
      hipLaunchKernelGGL(joint_loss_finalize_kernel<true>, dim3(M), dim3(64), 0, s, M, T, spT, row, col, g_spT);
    else
      hipLaunchKernelGGL(joint_loss_finalize_kernel<false>, dim3(M), dim3(64), 0, s, M, T, spT, row, col, g_spT);
  }
  SKGS_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
