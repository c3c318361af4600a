// point_knn.hip -- exact K nearest neighbours among 3-D points, for tables too large for a blind scan: the Gaussians' own
// neighbour table (networks/sk_gs.py:1342-1355 `update_gs_knn`: P x P, K = 21, rebuilt after every densify / prune event) and
// `knn_points` over all Gaussians (sk_gs.py:1365).  P = 1e5 is 1e10 candidate pairs if scanned blindly; here the data are put in
// Z-order, cut into blocks of 64 consecutive points with one bounding box each, and a wave of 64 queries (neighbours in space:
// the queries are walked in the same order) visits only the blocks whose box can still hold a neighbour of one of its lanes.
//
//   bbox    bounding box of the finite data coordinates (integer atomics on order-preserving bit patterns: deterministic)
//   codes   63-bit Morton code of every point over that box (21 bits per axis), value = its row
//   sort    rocprim radix sort of (code, row) pairs (header-only; scratch from the caller's workspace, no allocation, no sync)
//   build   sorted copy [x, y, z, row] and the box of every block of 64
//   search  one lane per query, the K best kept sorted in registers by (distance, row) with the ballot + VOP3-select
//           network of sp_knn.hip (`topk_insert_lex`), the insertion skipped wave-wide when no lane's candidate enters
//
// Exactness.  The distance is the oracle's `dx*dx + dy*dy + dz*dz`, fp32, left to right, no contraction; rows ascend by
// (distance, row), ties to the lower row -- the list's order does not depend on the order the candidates arrive in, so the
// Z-order, the sort and the pruning are invisible in the result.  The skip test needs no safety margin: the box distance is
// formed by the SAME operation sequence from per-axis gaps g = max(0, blo - qhi, qlo - bhi), each ONE rounded subtraction.
// For any query q in the wave's box and point p in the block's box the real |q - p| per axis is >= the real gap, rounding is
// monotone, so fl(|q - p|) >= g, fl(d * d) >= fl(g * g), and the two left-to-right sums keep that order term by term: the box
// distance is <= the computed distance of every pair.  A block is skipped only when its box distance is GREATER than the
// largest K-th distance among the wave's lanes ("equal" is visited: an equal distance with a lower row still enters).
// A comparison with a NaN (non-finite coordinates) is false, i.e. "visit": such rows cost time, never correctness of the others,
// and every loop runs over a fixed number of blocks.
#pragma clang fp contract(off)
#include <algorithm>
#include <cstdint>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "skgs_common.h"

namespace skgs {
namespace {

constexpr int PK_BLOCK   = 64;   // data points per block = candidates staged per visit (one per lane)
constexpr int PK_THREADS = 256;  // four independent waves per workgroup

__device__ __forceinline__ float pk_sel(uint64_t m, float t, float f) {  // (see sp_knn.hip::sel: the VOP3 select)
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m));
  return r;
}
__device__ __forceinline__ int pk_sel(uint64_t m, int t, int f) {
  int r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m));
  return r;
}
template <int KCAP>
__device__ __forceinline__ void pk_insert_lex(float (&bd)[KCAP], int (&bi)[KCAP], float d, int id) {
  uint64_t lt[KCAP];
#pragma unroll
  for (int k = 0; k < KCAP; ++k)
    lt[k] = __builtin_amdgcn_ballot_w64(d < bd[k]) | (__builtin_amdgcn_ballot_w64(d == bd[k]) & __builtin_amdgcn_ballot_w64(id < bi[k]));
#pragma unroll
  for (int k = KCAP - 1; k >= 1; --k) {
    bi[k] = pk_sel(lt[k - 1], bi[k - 1], pk_sel(lt[k], id, bi[k]));
    bd[k] = pk_sel(lt[k - 1], bd[k - 1], pk_sel(lt[k], d, bd[k]));
  }
  bi[0] = pk_sel(lt[0], id, bi[0]);
  bd[0] = pk_sel(lt[0], d, bd[0]);
}

// order-preserving map float -> uint32 (for integer atomicMin / atomicMax)
__device__ __forceinline__ uint32_t f_ordered(float f) {
  const uint32_t u = f2u(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f_unordered(uint32_t o) { return u2f((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
__device__ __forceinline__ bool pk_finite(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

// bbox words: [0..2] min (ordered), [3..5] max (ordered)
__global__ void __launch_bounds__(64) pk_bbox_init_kernel(uint32_t* __restrict__ bbox) {
  if (threadIdx.x < 8) bbox[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

__global__ void __launch_bounds__(256) pk_bbox_kernel(int n, const float* __restrict__ pts, uint32_t* __restrict__ bbox) {
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = pts[(size_t) 3 * i + c];
      if (pk_finite(v)) lo[c] = fminf(lo[c], v), hi[c] = fmaxf(hi[c], v);
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], s));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], s));
    }
  }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (lo[c] <= hi[c]) {  // (a wave that saw a finite value)
        atomicMin(&bbox[c], f_ordered(lo[c]));
        atomicMax(&bbox[3 + c], f_ordered(hi[c]));
      }
    }
}

__device__ __forceinline__ uint64_t spread21(uint32_t v) {  // bit i -> bit 3 i
  uint64_t x = v & 0x1fffffu;
  x = (x | (x << 32)) & 0x001f00000000ffffull;
  x = (x | (x << 16)) & 0x001f0000ff0000ffull;
  x = (x | (x << 8)) & 0x100f00f00f00f00full;
  x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

// Morton codes over the DATA's box (query points outside it are clamped onto it: the order is a matter of speed only)
__global__ void __launch_bounds__(256) pk_codes_kernel(int n, const float* __restrict__ pts, const uint32_t* __restrict__ bbox,
    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t code = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t olo = bbox[c], ohi = bbox[3 + c];
    float q = 0.f;
    if (olo <= ohi) {  // (else: no finite coordinate on this axis)
      const float lo = f_unordered(olo), ext = f_unordered(ohi) - lo;
      const float scale = (ext > 0.f && pk_finite(ext)) ? 2097151.f / ext : 0.f;
      q = (pts[(size_t) 3 * i + c] - lo) * scale;
    }
    q = fminf(fmaxf(q, 0.f), 2097151.f);  // (fmaxf(NaN, 0) = 0)
    code |= spread21((uint32_t) q) << c;
  }
  keys[i] = code;
  vals[i] = (uint32_t) i;
}

// one wave per block of 64 sorted points: the sorted copy and the block's box
__global__ void __launch_bounds__(PK_THREADS) pk_build_kernel(int n, const float* __restrict__ pts, const uint32_t* __restrict__ perm,
    float4* __restrict__ sorted, float4* __restrict__ boxes) {
  const int i = blockIdx.x * PK_THREADS + threadIdx.x;  // (n is padded to whole waves by the grid; lanes beyond n only reduce)
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  if (i < n) {
    const uint32_t r = min(perm[i], (uint32_t) (n - 1));
    const float x = pts[(size_t) 3 * r], y = pts[(size_t) 3 * r + 1], z = pts[(size_t) 3 * r + 2];
    sorted[i] = make_float4(x, y, z, u2f(r));
    lo[0] = hi[0] = x, lo[1] = hi[1] = y, lo[2] = hi[2] = z;  // (fminf / fmaxf below drop a NaN against a number)
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], s));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], s));
    }
  const int b = i / PK_BLOCK;
  if ((threadIdx.x & 63) == 0 && b * PK_BLOCK < n) {
    boxes[2 * b]     = make_float4(lo[0], lo[1], lo[2], 0.f);
    boxes[2 * b + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
}

// wave maximum of non-negative values (or -inf: "no value"; then the result is >= 0, which only means "visit boxes at distance 0")
__device__ __forceinline__ float wave_max_nonneg(float v) {
  v = fmaxf(v, dpp_mov<0x111, 0xf, 0xf, true>(v));   // row_shr:1 (lanes shifted in from outside read 0)
  v = fmaxf(v, dpp_mov<0x112, 0xf, 0xf, true>(v));
  v = fmaxf(v, dpp_mov<0x114, 0xf, 0xf, true>(v));
  v = fmaxf(v, dpp_mov<0x118, 0xf, 0xf, true>(v));   // lane 15 of each row = row maximum
  v = fmaxf(v, dpp_mov<0x142, 0xa, 0xf, false>(v));  // row_bcast:15 into rows 1, 3
  v = fmaxf(v, dpp_mov<0x143, 0xc, 0xf, false>(v));  // row_bcast:31 into rows 2, 3: lane 63 = the wave's
  return u2f(__builtin_amdgcn_readlane(f2u(v), 63));
}

// squared distance between two boxes by the candidates' own operation sequence (see the header: <= every pair's distance)
__device__ __forceinline__ float box_dist2(const float (&qlo)[3], const float (&qhi)[3], const float4& blo, const float4& bhi) {
  const float gx = fmaxf(0.f, fmaxf(blo.x - qhi[0], qlo[0] - bhi.x));
  const float gy = fmaxf(0.f, fmaxf(blo.y - qhi[1], qlo[1] - bhi.y));
  const float gz = fmaxf(0.f, fmaxf(blo.z - qhi[2], qlo[2] - bhi.z));
  float d = gx * gx;
  d += gy * gy;
  d += gz * gz;
  return d;
}

template <int KCAP>
__global__ void __launch_bounds__(PK_THREADS) pk_search_kernel(int n_data, int n_query, int K, int self_query,
    const float* __restrict__ queries, const uint32_t* __restrict__ qperm, const float4* __restrict__ sorted,
    const float4* __restrict__ boxes, int64_t* __restrict__ out_idx, float* __restrict__ out_dist2, float* __restrict__ out_dist) {
  __shared__ __attribute__((aligned(16))) float4 s_all[PK_THREADS];
  const int lane = threadIdx.x & 63;
  float4* s_pts  = s_all + (threadIdx.x - lane);  // this wave's 64 candidates
  const int w    = (blockIdx.x * PK_THREADS + threadIdx.x) >> 6;  // the wave's position in the query order
  if (w * PK_BLOCK >= n_query) return;                             // (whole waves leave: wave-uniform)
  const int nblk = (n_data + PK_BLOCK - 1) / PK_BLOCK;
  const int qpos = w * PK_BLOCK + lane;
  const bool live = qpos < n_query;
  const uint32_t qrow = min(qperm[min(qpos, n_query - 1)], (uint32_t) (n_query - 1));  // (lanes beyond the end follow the last query)
  const float qx = queries[(size_t) 3 * qrow], qy = queries[(size_t) 3 * qrow + 1], qz = queries[(size_t) 3 * qrow + 2];
  const bool finite = pk_finite(qx) && pk_finite(qy) && pk_finite(qz);  // (other rows: unspecified neighbours, they steer nothing)

  float qlo[3], qhi[3];
  {
    const float inf = __builtin_inff();
    qlo[0] = finite ? qx : inf, qlo[1] = finite ? qy : inf, qlo[2] = finite ? qz : inf;
    qhi[0] = finite ? qx : -inf, qhi[1] = finite ? qy : -inf, qhi[2] = finite ? qz : -inf;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) {
        qlo[c] = fminf(qlo[c], __shfl_xor(qlo[c], s));
        qhi[c] = fmaxf(qhi[c], __shfl_xor(qhi[c], s));
      }
      qlo[c] = u2f(__builtin_amdgcn_readfirstlane(f2u(qlo[c])));
      qhi[c] = u2f(__builtin_amdgcn_readfirstlane(f2u(qhi[c])));
    }
  }

  float bd[KCAP];
  int bi[KCAP];
#pragma unroll
  for (int k = 0; k < KCAP; ++k) bd[k] = __builtin_inff(), bi[k] = 0x7fffffff;  // (loses every (distance, row) comparison)

  // the 64 points of block b through LDS, every lane against every one of them
  auto scan_block = [&](int b) {
    const int p = b * PK_BLOCK + lane;
    // (rows beyond the end of a partial block: NaN coordinates, never inserted)
    s_pts[lane] = p < n_data ? sorted[p] : make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), 0.f);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    bool any = false;
#pragma unroll 2
    for (int j = 0; j < PK_BLOCK; ++j) {
      const float4 c = s_pts[j];  // (broadcast read)
      const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
      float d = dx * dx;
      d += dy * dy;
      d += dz * dz;
      // "<=": an equal distance with a lower row still displaces the list's last entry
      // (the lane's bound is its KCAP-th distance: for K < KCAP -- K = 17..20 on 21 slots -- looser than its K-th, still exact;
      // a bound at slot K - 1 would be a dynamic register index in the innermost loop)
      const uint64_t m = __builtin_amdgcn_ballot_w64(d <= bd[KCAP - 1]);
      if (m != 0) {  // (a lane whose candidate cannot enter inserts a NaN: every comparison fails, nothing moves)
        pk_insert_lex<KCAP>(bd, bi, pk_sel(m, d, __builtin_nanf("")), (int) f2u(c.w));
        any = true;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // (the next visit overwrites the staging rows)
    return any;
  };
  auto wave_bound = [&]() { return wave_max_nonneg(finite ? bd[KCAP - 1] : -__builtin_inff()); };

  // ---- home: the block the wave's own points are in (self query: the queries ARE the blocks), else the block nearest to its box
  int home = w;
  if (!self_query) {
    float best = __builtin_inff();
    int arg = 0x7fffffff;
    for (int c0 = 0; c0 < nblk; c0 += 64) {
      const int b = c0 + lane;
      if (b < nblk) {
        const float d = box_dist2(qlo, qhi, boxes[2 * b], boxes[2 * b + 1]);
        if (d < best) best = d, arg = b;
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const float od = __shfl_xor(best, s);
      const int oa   = __shfl_xor(arg, s);
      if (od < best || (od == best && oa < arg)) best = od, arg = oa;
    }
    home = __builtin_amdgcn_readfirstlane(arg);
  }
  home = max(0, min(home, nblk - 1));  // (no finite box at all: any block)
  const int h0 = max(home - 1, 0), h1 = min(home + 1, nblk - 1);
  scan_block(home);
  if (h0 != home) scan_block(h0);
  if (h1 != home) scan_block(h1);
  float bound = wave_bound();

  // ---- every other block whose box is within the bound: 64 boxes per step, one per lane; the bound shrinks as lists improve
  for (int c0 = 0; c0 < nblk; c0 += 64) {
    const int b = c0 + lane;
    const bool cand = b < nblk && (b < h0 || b > h1);
    float d = 0.f;
    if (cand) d = box_dist2(qlo, qhi, boxes[2 * b], boxes[2 * b + 1]);
    uint64_t m = __builtin_amdgcn_ballot_w64(cand && !(d > bound));
    while (m != 0) {
      const int j = __builtin_ctzll(m);
      if (scan_block(c0 + j)) bound = wave_bound();
      m = __builtin_amdgcn_ballot_w64(cand && !(d > bound)) & ~((2ull << j) - 1ull);  // (j = 63: 2 << 63 = 0, mask all)
    }
  }

  if (!live) return;
  int64_t* oi = out_idx + (size_t) qrow * K;
#pragma unroll
  for (int k = 0; k < KCAP; ++k)
    if (k < K) {
      const bool none = bi[k] == 0x7fffffff;  // fewer than K data points
      oi[k] = none ? (int64_t) -1 : (int64_t) bi[k];
      if (out_dist2) out_dist2[(size_t) qrow * K + k] = bd[k];
      if (out_dist) out_dist[(size_t) qrow * K + k] = sqrtf(bd[k]);
    }
}

struct PkLayout {
  size_t bbox, keys_a, keys_b, vals_a, vals_b, sorted, boxes, sort_tmp, sort_tmp_bytes, total;
};

hipError_t pk_sort(void* tmp, size_t& tmp_bytes, uint64_t* ka, uint64_t* kb, uint32_t* va, uint32_t* vb, int n, hipStream_t s) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, ka, kb, va, vb, (size_t) n, 0u, 63u, s, false);
}

// scratch of the sort for n pairs (rocprim's own answer; it asks the device for its architecture)
bool pk_sort_bytes(int n, size_t& bytes, hipStream_t s) {
  bytes = 0;
  if (n <= 0) return true;
  return pk_sort(nullptr, bytes, nullptr, nullptr, nullptr, nullptr, n, s) == hipSuccess;
}

// `s`: the stream the sort will run on (rocprim sizes its scratch for that stream's device)
bool pk_layout(int n_data, int n_query, PkLayout& L, hipStream_t s) {
  const size_t N = (size_t) std::max(std::max(n_data, n_query), 1);
  const size_t nblk = (std::max(n_data, 1) + PK_BLOCK - 1) / PK_BLOCK;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
  L.bbox   = take(32);
  L.keys_a = take(N * 8);
  L.keys_b = take(N * 8);
  L.vals_a = take(N * 4);
  L.vals_b = take(N * 4);
  L.sorted = take((size_t) std::max(n_data, 1) * 16);
  L.boxes  = take(nblk * 32);
  size_t for_data = 0, for_queries = 0;  // (the sort runs once per cloud: the larger of its two answers)
  const bool ok = pk_sort_bytes(n_data, for_data, s) && pk_sort_bytes(n_query, for_queries, s);
  L.sort_tmp_bytes = std::max(for_data, for_queries);
  L.sort_tmp = take(L.sort_tmp_bytes);
  L.total = at;
  return ok;
}

}  // namespace
}  // namespace skgs

using namespace skgs;

extern "C" {

size_t skgs_point_knn_workspace_bytes(int32_t n_data, int32_t n_query) {
  if (n_data < 0 || n_query < 0) return 0;
  PkLayout L;
  pk_layout(n_data, n_query, L, nullptr);  // (sized for the current device; without a device the sort's share is reported as 0: the call itself then refuses)
  return L.total;
}

int skgs_point_knn(int32_t n_data, const float* data, int32_t n_query, const float* queries, int32_t K, int64_t* out_idx,
    float* out_dist2, float* out_dist, void* workspace, size_t workspace_bytes, skgs_stream_t stream) {
  SKGS_REQUIRE(n_data >= 0 && n_query >= 0, "point_knn: negative point count");
  SKGS_REQUIRE(K >= 1 && K <= 32, "point_knn: need 1 <= K <= 32");
  if (n_data == 0 || n_query == 0) return 0;
  SKGS_REQUIRE(data && out_idx, "point_knn: NULL argument");
  const bool self_query = queries == nullptr || (queries == data && n_query == n_data);
  SKGS_REQUIRE(queries || n_query == n_data, "point_knn: a self query (queries = NULL) needs n_query = n_data");
  hipStream_t s = (hipStream_t) stream;
  PkLayout L;
  SKGS_REQUIRE(pk_layout(n_data, n_query, L, s), "point_knn: the sort's scratch size could not be determined (no HIP device?)");
  SKGS_REQUIRE(workspace && workspace_bytes >= L.total, "point_knn: workspace too small (skgs_point_knn_workspace_bytes)");
  SKGS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "point_knn: workspace must be 16-byte aligned");
  char* base       = reinterpret_cast<char*>(workspace);
  uint32_t* bbox   = reinterpret_cast<uint32_t*>(base + L.bbox);
  uint64_t* keys_a = reinterpret_cast<uint64_t*>(base + L.keys_a);
  uint64_t* keys_b = reinterpret_cast<uint64_t*>(base + L.keys_b);
  uint32_t* vals_a = reinterpret_cast<uint32_t*>(base + L.vals_a);
  uint32_t* vals_b = reinterpret_cast<uint32_t*>(base + L.vals_b);
  float4* sorted   = reinterpret_cast<float4*>(base + L.sorted);
  float4* boxes    = reinterpret_cast<float4*>(base + L.boxes);
  void* sort_tmp   = base + L.sort_tmp;
  const int nblk   = (n_data + PK_BLOCK - 1) / PK_BLOCK;
  {
    ProfScope prof(K_POINT_KNN_SORT, s);
    hipLaunchKernelGGL(pk_bbox_init_kernel, dim3(1), dim3(64), 0, s, bbox);
    hipLaunchKernelGGL(pk_bbox_kernel, dim3(std::min((n_data + 255) / 256, 1024)), dim3(256), 0, s, n_data, data, bbox);
    hipLaunchKernelGGL(pk_codes_kernel, dim3((n_data + 255) / 256), dim3(256), 0, s, n_data, data, bbox, keys_a, vals_a);
    SKGS_CHECK_HIP(hipGetLastError());
    size_t tmp_bytes = L.sort_tmp_bytes;
    SKGS_CHECK_HIP(pk_sort(sort_tmp, tmp_bytes, keys_a, keys_b, vals_a, vals_b, n_data, s));
  }
  {
    ProfScope prof(K_POINT_KNN_BUILD, s);
    hipLaunchKernelGGL(pk_build_kernel, dim3((nblk * PK_BLOCK + PK_THREADS - 1) / PK_THREADS), dim3(PK_THREADS), 0, s, n_data, data,
        vals_b, sorted, boxes);
    SKGS_CHECK_HIP(hipGetLastError());
  }
  if (!self_query) {  // the queries in the same order (their own sort; the data's permutation is no longer needed)
    ProfScope prof(K_POINT_KNN_SORT, s);
    hipLaunchKernelGGL(pk_codes_kernel, dim3((n_query + 255) / 256), dim3(256), 0, s, n_query, queries, bbox, keys_a, vals_a);
    SKGS_CHECK_HIP(hipGetLastError());
    size_t tmp_bytes = L.sort_tmp_bytes;
    SKGS_CHECK_HIP(pk_sort(sort_tmp, tmp_bytes, keys_a, keys_b, vals_a, vals_b, n_query, s));
  }
  {
    ProfScope prof(K_POINT_KNN_SEARCH, s);
    const float* q = queries ? queries : data;
    const dim3 grid(((n_query + PK_BLOCK - 1) / PK_BLOCK * PK_BLOCK + PK_THREADS - 1) / PK_THREADS), block(PK_THREADS);
#define SKGS_PK(KCAP_)                                                                                                        \
  hipLaunchKernelGGL((pk_search_kernel<KCAP_>), grid, block, 0, s, n_data, n_query, K, self_query ? 1 : 0, q, vals_b, sorted, \
      boxes, out_idx, out_dist2, out_dist)
    if (K <= 4) SKGS_PK(4); else if (K <= 8) SKGS_PK(8); else if (K <= 16) SKGS_PK(16); else if (K <= 21) SKGS_PK(21); else SKGS_PK(32);
#undef SKGS_PK
    SKGS_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
