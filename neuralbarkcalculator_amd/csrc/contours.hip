// How far the contours of a label map lie from the contours of its labelled mask (nbc_contour_distances, include/nbc.h): per
// image and set the number of source and destination contour pixels, the sum and the maximum of the squared distances from
// every source contour pixel to the nearest destination contour pixel, a histogram of the distances rounded up to whole
// pixels, and the float64 sum of the distances.  The integers are exact against the host restatement
// (neuralbarkcalculator_amd/contours.py: contours_cpu); the distance transform is the exact two-pass one (columns, then rows).
//
// Class maps: the labels (1, 2; anything else is no class) and the grey dual by nbc_confusion's rule (target_class,
// reduce.hpp).  A pixel is on the contour of class c iff it has class c and a 4-neighbour inside the image does not.
// Set s = 2 (c - 1) + dir: dir 0 goes from the output's contour to the target's, dir 1 back.  The contour kind that is the
// source of set s is the destination of set s ^ 1, so four kinds serve as four sources and four destinations.
//   contour_mark      a block per tile of 256 x 16 pixels: both class maps of the tile and its one-pixel halo into LDS as one
//                     byte per pixel, then a thread per column of the tile: one mark byte per pixel whose bit s says "source
//                     of set s"; the four counts n of the tile (wave_sum, the waves through LDS) make one integer atomic per
//                     set and block into the rows' n words
//   column_distance   a block per (image, 64 columns), lanes along x, 16 segments of rows: a thread finds the first and the
//                     last contour row of each kind in its segment; through LDS it learns the last one above and the first
//                     one below its segment; a sweep down and a sweep up over the segment then leave per pixel and kind the
//                     vertical distance to the nearest contour pixel of the column, u16, 65535 = none.  The four kinds of
//                     a pixel are one 8-byte word, so both sweeps store 512 contiguous bytes per wave
//   row_min           a block per (image, 8 rows), a row at a time: the row's 4 x W column distances into LDS (u16, squared
//                     when read) and its work items -- (x, set) for every source pixel x of a set whose destination exists,
//                     compacted by a prefix sum over the threads, so that every lane scans: best = g2(x), and for
//                     k = 1, 2, ... while k < W and k * k < best: best = min(best, k * k + min(g2(x - k), g2(x + k))).
//                     The loop ends after at most W steps whatever the data.  Sums, maxima and bins are integer atomics, one
//                     per block and used cell (bins below kLocalBins through an LDS histogram); the distances are summed in
//                     f64 in an order the row alone fixes (the items in their order round-robin over the threads, wave_sum,
//                     the waves in order) into one partial per (image, set, row)
//   contour_finish    a wave per (image, set): the row partials in the order pixel_ce_finish adds its tiles, and m
// The rows are zeroed by a memset in front: every word of an image's rows and sum_d is written on every call.  The float
// sums' order depends on the image alone (its shape and where its contours lie), never on the batch, the stream or the
// timing, so an image's outputs have the same bits alone, in any batch and on any stream.
#include "nbc_ctx.hpp"
#include "nbc_kernels.hpp"
#include "reduce.hpp"

namespace nbc {
namespace {

using u64 = unsigned long long;

constexpr int kSets = NBC_CONTOUR_SETS;
constexpr int kHead = NBC_CONTOUR_HEAD;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMarkRows = 16;                         // rows of a contour_mark tile
constexpr int kSegs = 16;                             // row segments of a column_distance block
constexpr int kRowsPerBlock = 8;                      // rows a row_min block takes, one after the other
constexpr int kLocalBins = kThreads / kSets;          // 64 bins per set in LDS: a thread flushes one
constexpr unsigned kNone = 65535u;                    // no contour pixel of the kind in this column
constexpr unsigned kFar = 0x40000000u;                // its square: above every d2 (< 2^26), and kFar + 4095^2 fits 32 bits
constexpr int kSweep = 8;                             // rows whose loads a sweep issues together
constexpr unsigned kOutside = 0xffu;                  // the class byte of a pixel outside the image
constexpr int kAbove = -(1 << 20), kBelow = 1 << 20;  // "no contour row": far above and far below every image

template <typename L>
__device__ __forceinline__ unsigned output_class(L v) { return v == (L)1 ? 1u : v == (L)2 ? 2u : 0u; }

template <typename L>
__global__ __launch_bounds__(kThreads) void contour_mark_kernel(const L* __restrict__ labels, const unsigned char* __restrict__ grey,
                                                                int H, int W, unsigned char* __restrict__ mark,
                                                                u64* __restrict__ rows, int row_len) {
  constexpr int kPitch = kThreads + 2;
  __shared__ unsigned char cls[kMarkRows + 2][kPitch];   // output class | target class << 2 of the tile and its halo
  __shared__ unsigned cnt[kWaves][kSets];
  const int tid = threadIdx.x, x0 = blockIdx.x * kThreads, y0 = blockIdx.y * kMarkRows;
  const size_t img = (size_t)blockIdx.z * H * W;
  for (int i = tid; i < (kMarkRows + 2) * kPitch; i += kThreads) {
    const int r = i / kPitch, c = i - r * kPitch;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    unsigned v = kOutside;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t p = img + (size_t)y * W + x;
      v = output_class(labels[p]) | (target_class(grey[p]) << 2);
    }
    cls[r][c] = (unsigned char)v;
  }
  __syncthreads();
  unsigned n[kSets] = {0, 0, 0, 0};
  const int x = x0 + tid;
  if (x < W) {
    for (int r = 1; r <= kMarkRows && y0 + r - 1 < H; ++r) {
      const unsigned c = cls[r][tid + 1], o = c & 3u, t = c >> 2;
      const unsigned side[4] = {cls[r][tid], cls[r][tid + 2], cls[r - 1][tid + 1], cls[r + 1][tid + 1]};
      bool oe = false, te = false;                    // a 4-neighbour inside the image of another class
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        oe |= side[k] != kOutside && (side[k] & 3u) != o;
        te |= side[k] != kOutside && (side[k] >> 2) != t;
      }
      unsigned bits = 0;
      if (o && oe) bits |= 1u << (2 * (o - 1));
      if (t && te) bits |= 2u << (2 * (t - 1));
      mark[img + (size_t)(y0 + r - 1) * W + x] = (unsigned char)bits;
#pragma unroll
      for (int s = 0; s < kSets; ++s) n[s] += (bits >> s) & 1u;
    }
  }
#pragma unroll
  for (int s = 0; s < kSets; ++s) {
    const unsigned c = wave_sum(n[s]);
    if ((tid & 63) == 0) cnt[tid >> 6][s] = c;
  }
  __syncthreads();
  if (tid < kSets) {
    unsigned c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += cnt[w][tid];
    if (c) atomicAdd(&rows[((size_t)blockIdx.z * kSets + tid) * row_len], (u64)c);
  }
}

__global__ __launch_bounds__(64 * kSegs) void column_distance_kernel(const unsigned char* __restrict__ mark, int H, int W,
                                                                     ushort4* __restrict__ dist) {
  __shared__ int last_in[kSegs][kSets][64];           // per segment, kind and column: its last contour row, its first one
  __shared__ int first_in[kSegs][kSets][64];
  const int cx = threadIdx.x, seg = threadIdx.y, x = blockIdx.x * 64 + cx;
  const bool inside = x < W;
  const int per = (H + kSegs - 1) / kSegs, ya = seg * per, yb = min(H, ya + per);   // this thread's rows: ya .. yb - 1
  const size_t col = (size_t)blockIdx.y * H * W + (inside ? x : 0);
  const unsigned char* m = mark + col;
  ushort4* g = dist + col;
  int last[kSets], first[kSets];
#pragma unroll
  for (int s = 0; s < kSets; ++s) {
    last[s] = kAbove;
    first[s] = kBelow;
  }
  if (inside) {
    for (int y0 = ya; y0 < yb; y0 += kSweep) {
      unsigned b[kSweep];
#pragma unroll
      for (int i = 0; i < kSweep; ++i) b[i] = y0 + i < yb ? m[(size_t)(y0 + i) * W] : 0u;
#pragma unroll
      for (int i = 0; i < kSweep; ++i)
#pragma unroll
        for (int s = 0; s < kSets; ++s)
          if ((b[i] >> s) & 1u) {                     // a padding row has no bit
            last[s] = y0 + i;
            first[s] = min(first[s], y0 + i);
          }
    }
  }
#pragma unroll
  for (int s = 0; s < kSets; ++s) {
    last_in[seg][s][cx] = last[s];
    first_in[seg][s][cx] = first[s];
  }
  __syncthreads();
  if (!inside) return;
#pragma unroll
  for (int s = 0; s < kSets; ++s) {
    last[s] = kAbove;                                 // the last contour row above the segment, the first one below it
    first[s] = kBelow;
    for (int k = 0; k < seg; ++k) last[s] = max(last[s], last_in[k][s][cx]);
    for (int k = seg + 1; k < kSegs; ++k) first[s] = min(first[s], first_in[k][s][cx]);
  }
  for (int y0 = ya; y0 < yb; y0 += kSweep) {          // down: the distance to the nearest one at or above
    unsigned b[kSweep];
#pragma unroll
    for (int i = 0; i < kSweep; ++i) b[i] = y0 + i < yb ? m[(size_t)(y0 + i) * W] : 0u;
#pragma unroll
    for (int i = 0; i < kSweep; ++i) {
      const int y = y0 + i;
      if (y >= yb) break;
      unsigned d[kSets];
#pragma unroll
      for (int s = 0; s < kSets; ++s) {
        if ((b[i] >> s) & 1u) last[s] = y;
        d[s] = last[s] < 0 ? kNone : (unsigned)(y - last[s]);
      }
      g[(size_t)y * W] = make_ushort4((unsigned short)d[0], (unsigned short)d[1], (unsigned short)d[2], (unsigned short)d[3]);
    }
  }
  for (int y0 = yb - 1; y0 >= ya; y0 -= kSweep) {     // up: the smaller of that and the distance to the nearest one below
    unsigned b[kSweep];
    ushort4 v[kSweep];
#pragma unroll
    for (int i = 0; i < kSweep; ++i) {
      const bool in = y0 - i >= ya;
      b[i] = in ? m[(size_t)(y0 - i) * W] : 0u;
      v[i] = in ? g[(size_t)(y0 - i) * W] : make_ushort4(0, 0, 0, 0);   // this thread's own stores of the sweep down
    }
#pragma unroll
    for (int i = 0; i < kSweep; ++i) {
      const int y = y0 - i;
      if (y < ya) break;
      const unsigned down[kSets] = {v[i].x, v[i].y, v[i].z, v[i].w};
      unsigned d[kSets];
#pragma unroll
      for (int s = 0; s < kSets; ++s) {
        if ((b[i] >> s) & 1u) first[s] = y;
        const unsigned up = first[s] >= H ? kNone : (unsigned)(first[s] - y);
        d[s] = up < down[s] ? up : down[s];
      }
      g[(size_t)y * W] = make_ushort4((unsigned short)d[0], (unsigned short)d[1], (unsigned short)d[2], (unsigned short)d[3]);
    }
  }
}

__device__ __forceinline__ unsigned squared(unsigned g) { return g == kNone ? kFar : g * g; }

// ceil(sqrt(d2)) of an integer, exactly: isqrt(d2 - 1) + 1, the float root corrected on the integers
__device__ __forceinline__ unsigned ceil_sqrt(unsigned d2) {
  if (d2 == 0u) return 0u;
  const unsigned v = d2 - 1u;
  unsigned r = (unsigned)sqrt((double)v);
  while ((u64)r * r > v) --r;
  while ((u64)(r + 1u) * (r + 1u) <= v) ++r;
  return r + 1u;
}

__global__ __launch_bounds__(kThreads) void row_min_kernel(const unsigned char* __restrict__ mark, const ushort4* __restrict__ dist,
                                                           int H, int W, u64* __restrict__ rows, int row_len, int bins,
                                                           double* __restrict__ partial) {
  extern __shared__ unsigned short sg[];              // [kSets][W]: the row's column distances per kind; then item[2 W]
  __shared__ unsigned hist[kSets][kLocalBins];
  __shared__ unsigned wtot[kWaves];
  __shared__ double dred[kWaves][kSets];
  __shared__ u64 sred[kWaves][kSets];
  __shared__ unsigned mred[kWaves][kSets];
  unsigned short* item = sg + (size_t)kSets * W;      // the row's (x | set << 12) work items: at most two sets per pixel
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.y;
  u64* R = rows + (size_t)n * kSets * row_len;
  hist[tid / kLocalBins][tid % kLocalBins] = 0u;
  unsigned live = 0;                                  // bit s: the set's destination exists (m of set s is n of set s ^ 1)
#pragma unroll
  for (int s = 0; s < kSets; ++s) live |= (R[(size_t)(s ^ 1) * row_len] != 0ull ? 1u : 0u) << s;

  u64 s2[kSets] = {0, 0, 0, 0};
  unsigned mx[kSets] = {0, 0, 0, 0};
  for (int r = 0; r < kRowsPerBlock; ++r) {
    const int y = blockIdx.x * kRowsPerBlock + r;
    if (y >= H) break;                                // uniform over the block
    const size_t row = ((size_t)n * H + y) * W;
    double sd[kSets] = {0.0, 0.0, 0.0, 0.0};
    if (live) {                                       // uniform over the block
      // the items of the row in an order the row alone fixes: by thread, a thread's pixels by x, a pixel's sets by s
      unsigned mine = 0;
      for (int x = tid; x < W; x += kThreads) {
        const ushort4 v = dist[row + x];
        sg[x] = v.x;
        sg[W + x] = v.y;
        sg[2 * W + x] = v.z;
        sg[3 * W + x] = v.w;
        mine += (unsigned)__popc(mark[row + x] & live);
      }
      unsigned upto = mine;                           // inclusive scan over the wave's lanes
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned below = (unsigned)__shfl_up((int)upto, off, 64);
        if (lane >= off) upto += below;
      }
      if (lane == 63) wtot[wave] = upto;
      __syncthreads();                                // also orders the first row behind the cleared histogram
      unsigned at = upto - mine, total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        if (w < wave) at += wtot[w];
        total += wtot[w];
      }
      for (int x = tid; x < W; x += kThreads) {
        const unsigned b = mark[row + x] & live;
#pragma unroll
        for (int s = 0; s < kSets; ++s)
          if ((b >> s) & 1u) item[at++] = (unsigned short)(x | (s << 12));
      }
      __syncthreads();
      for (unsigned i = tid; i < total; i += kThreads) {
        const int x = item[i] & 4095, s = item[i] >> 12;
        const unsigned short* g = sg + (size_t)(s ^ 1) * W;
        unsigned best = squared(g[x]);
        for (int k = 1; k < W && (unsigned)(k * k) < best; ++k) {
          const unsigned k2 = (unsigned)(k * k);
          if (x - k >= 0) best = min(best, k2 + squared(g[x - k]));
          if (x + k < W) best = min(best, k2 + squared(g[x + k]));
        }
        // a destination pixel exists in some column q of the image, whose distance is finite in every row: the scan
        // reaches k = |x - q| unless a smaller best stops it, so best is finite here
        const double root = sqrt((double)best);
#pragma unroll
        for (int k = 0; k < kSets; ++k) {             // selects, not a run-time index into registers
          s2[k] += s == k ? best : 0u;
          mx[k] = max(mx[k], s == k ? best : 0u);
          sd[k] += s == k ? root : 0.0;
        }
        const unsigned k = ceil_sqrt(best);
        const int bin = k < (unsigned)(bins - 1) ? (int)k : bins - 1;
        if (bin < kLocalBins) atomicAdd(&hist[s][bin], 1u);
        else atomicAdd(&R[(size_t)s * row_len + kHead + bin], 1ull);
      }
    }
#pragma unroll
    for (int s = 0; s < kSets; ++s) {
      const double a = wave_sum(sd[s]);
      if (lane == 0) dred[wave][s] = a;
    }
    __syncthreads();                                  // the row's scans are done: sg, item and wtot may be overwritten
    if (tid < kSets) {
      double a = 0.0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) a += dred[w][tid];
      partial[((size_t)n * kSets + tid) * H + y] = a;
    }
    __syncthreads();                                  // dred is read: the next row may write it
  }
#pragma unroll
  for (int s = 0; s < kSets; ++s) {
    const u64 c = wave_sum(s2[s]);
    unsigned m = mx[s];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    if (lane == 0) {
      sred[wave][s] = c;
      mred[wave][s] = m;
    }
  }
  __syncthreads();
  if (tid < kSets) {
    u64 c = 0;
    unsigned m = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      c += sred[w][tid];
      m = max(m, mred[w][tid]);
    }
    if (c) atomicAdd(&R[(size_t)tid * row_len + 2], c);
    if (m) atomicMax(&R[(size_t)tid * row_len + 3], (u64)m);
  }
  const int hs = tid / kLocalBins, hb = tid % kLocalBins;
  const unsigned c = hist[hs][hb];                    // a used local bin is below bins: bin <= bins - 1
  if (c) atomicAdd(&R[(size_t)hs * row_len + kHead + hb], (u64)c);
}

__global__ __launch_bounds__(64) void contour_finish_kernel(const double* __restrict__ partial, int H, u64* __restrict__ rows,
                                                            int row_len, double* __restrict__ sum_d) {
  const size_t seg = blockIdx.x;                      // image * 4 + set
  const int lane = threadIdx.x;
  const double* p = partial + seg * H;
  double s = 0.0;
  for (int y = lane; y < H; y += 64) s += p[y];
  s = wave_sum(s);
  if (lane == 0) {
    sum_d[seg] = s;                                   // 0.0 where the set has no source or no destination
    rows[seg * row_len + 1] = rows[(seg ^ 1) * row_len];
  }
}

// The regions of the workspace (byte offsets, each 256-byte aligned) and its size: a mark byte per pixel, the four u16 column
// distances per pixel, and an f64 partial per (image, set, row).
struct ContoursLayout {
  size_t mark, dist, partial, total;
};
ContoursLayout contours_layout(int N, int H, int W) {
  const size_t px = (size_t)N * H * W;
  Carver ws;
  const size_t mark = ws.take(px), dist = ws.take(8 * px), partial = ws.take(8 * (size_t)N * kSets * H);
  return {mark, dist, partial, ws.offset};
}

bool contours_shape_ok(int N, int H, int W) {
  return N >= 1 && N <= 65535 && H >= 1 && H <= NBC_CONTOUR_MAX_SIDE && W >= 1 && W <= NBC_CONTOUR_MAX_SIDE;
}
constexpr int kContourMaxBins = 5793;         // ceil(hypot(4095, 4095)) + 1

}  // namespace
}  // namespace nbc

using namespace nbc;

extern "C" size_t nbc_contours_workspace_bytes(int N, int H, int W) {
  return contours_shape_ok(N, H, W) ? contours_layout(N, H, W).total : 0;
}

extern "C" int nbc_contour_distances(nbc_ctx* c, const void* labels_dev, int labels_dtype, const uint8_t* target_grey_dev, int N,
                                     int H, int W, int64_t* rows_dev, int bins, double* sum_d_dev, void* workspace_dev,
                                     size_t workspace_bytes, void* hip_stream) {
  constexpr const char* kWho = "nbc_contour_distances";
  if (!c || !labels_dev || !target_grey_dev || !rows_dev || !sum_d_dev || !workspace_dev)
    return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (!contours_shape_ok(N, H, W))
    return fail(kWho, NBC_ERR_INVALID, "bad shape: 1 <= N <= 65535, H and W in 1.." + std::to_string(NBC_CONTOUR_MAX_SIDE));
  if (bins < 2 || bins > kContourMaxBins) return fail(kWho, NBC_ERR_INVALID, "bins must lie in 2.." + std::to_string(kContourMaxBins));
  if (!label_dtype_ok(labels_dtype)) return fail(kWho, NBC_ERR_INVALID, "bad labels_dtype");
  const ContoursLayout lay = contours_layout(N, H, W);
  if (const int rc = check_workspace(kWho, workspace_dev, workspace_bytes, lay.total)) return rc;
  NBC_HIP(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace_dev);
  unsigned char* mark = ws + lay.mark;
  ushort4* dist = reinterpret_cast<ushort4*>(ws + lay.dist);
  double* partial = reinterpret_cast<double*>(ws + lay.partial);
  u64* R = reinterpret_cast<u64*>(rows_dev);
  const int row_len = kHead + bins;
  NBC_HIP(hipMemsetAsync(rows_dev, 0, sizeof(long long) * (size_t)N * kSets * row_len, s));
  const dim3 tiles((W + kThreads - 1) / kThreads, (H + kMarkRows - 1) / kMarkRows, N);
  if (labels_dtype == NBC_LABEL_I64)
    hipLaunchKernelGGL(contour_mark_kernel<long long>, tiles, dim3(kThreads), 0, s, static_cast<const long long*>(labels_dev),
                       target_grey_dev, H, W, mark, R, row_len);
  else
    hipLaunchKernelGGL(contour_mark_kernel<unsigned char>, tiles, dim3(kThreads), 0, s, static_cast<const unsigned char*>(labels_dev),
                       target_grey_dev, H, W, mark, R, row_len);
  hipLaunchKernelGGL(column_distance_kernel, dim3((W + 63) / 64, N), dim3(64, kSegs), 0, s, mark, H, W, dist);
  hipLaunchKernelGGL(row_min_kernel, dim3((H + kRowsPerBlock - 1) / kRowsPerBlock, N), dim3(kThreads),
                     sizeof(unsigned short) * (kSets + 2) * (size_t)W, s, mark, dist, H, W, R, row_len, bins, partial);
  hipLaunchKernelGGL(contour_finish_kernel, dim3(N * kSets), dim3(64), 0, s, partial, H, R, row_len, sum_d_dev);
  NBC_HIP(hipGetLastError());
  return NBC_OK;
}

