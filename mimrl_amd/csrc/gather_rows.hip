// mimrl_op_gather_rows: dst[a][r, :] = src[a][idx[r], :] for up to four arrays in ONE launch -- the shuffled batch upload of
// HipEngine.stage_batch / set_batch (text, audio, video and labels of a batch, gathered straight into an input set; no temporary).
//
// Work item = (destination row r, chunk c): a row of every array is cut into chunks of GR_CHUNK bytes (the last one partial), so that one
// long row (T * d_t * 4 = 150 KB at cfg2) spreads over many workgroups; the chunks of the arrays of one row are numbered one array after
// the other.  The grid strides over the items, so any workgroup count (max_workgroups) computes the same bytes.  idx[r] is one
// wave-uniform load per item.  An index outside [0, src_rows) is never used as an address: that destination row becomes NaN in every array
// (the convention of a non-class label in mimrl_op_class_loss).  Plain vector loads and stores whose waits the compiler places; no LDS,
// no accumulation (det.hip: nothing to flush behind it -- and it runs on the upload stream, where a flush must not run).
#include "common.h"

namespace mimrl {

constexpr int GR_THREADS = 256;
constexpr int GR_CHUNK = 16384;      // bytes of a row per work item: 4 x 16-byte vectors per lane
constexpr int GR_UNROLL = 4;         // loads in flight per lane

struct GatherRowsArgs {
  const char* src[4];
  char* dst[4];
  int64_t row_bytes[4];
  int32_t chunk0[5];                 // first chunk number of array a within a row; chunk0[n] = chunks per row
  int32_t width[4];                  // bytes per lane: 16, 8 or 4
  int32_t n;
  int32_t rows;
  int64_t src_rows;
  const int32_t* idx;
};

typedef uint32_t gr_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t gr_u32x2 __attribute__((ext_vector_type(2)));

template <class V> __device__ __forceinline__ V gr_nan();
template <> __device__ __forceinline__ uint32_t gr_nan<uint32_t>() { return 0x7fc00000u; }
template <> __device__ __forceinline__ gr_u32x2 gr_nan<gr_u32x2>() { return gr_u32x2{0x7fc00000u, 0x7fc00000u}; }
template <> __device__ __forceinline__ gr_u32x4 gr_nan<gr_u32x4>() { return gr_u32x4{0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0x7fc00000u}; }

// bytes [lo, hi) of one row: s = source row (nullptr: fill with NaN), d = destination row; both aligned to sizeof(V), as are lo and hi
template <class V>
__device__ __forceinline__ void gr_copy(const char* s, char* d, int64_t lo, int64_t hi) {
  constexpr int64_t W = sizeof(V);
  for (int64_t b = lo + (int64_t)threadIdx.x * W; b < hi; b += (int64_t)GR_THREADS * W * GR_UNROLL) {
    V v[GR_UNROLL];
#pragma unroll
    for (int k = 0; k < GR_UNROLL; ++k) {
      const int64_t o = b + (int64_t)k * GR_THREADS * W;
      v[k] = gr_nan<V>();
      if (s && o < hi) v[k] = __builtin_nontemporal_load(reinterpret_cast<const V*>(s + o));
    }
#pragma unroll
    for (int k = 0; k < GR_UNROLL; ++k) {
      const int64_t o = b + (int64_t)k * GR_THREADS * W;
      if (o < hi) *reinterpret_cast<V*>(d + o) = v[k];
    }
  }
}

__global__ void __launch_bounds__(GR_THREADS) gather_rows_kernel(GatherRowsArgs g) {
  const int per_row = g.chunk0[g.n];
  const int64_t items = (int64_t)g.rows * per_row;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int r = (int)(item / per_row);
    const int c = (int)(item - (int64_t)r * per_row);
    int a = 0;
    while (a + 1 < g.n && c >= g.chunk0[a + 1]) ++a;
    const int64_t i = g.idx[r];
    const int64_t rb = g.row_bytes[a];
    const int64_t lo = (int64_t)(c - g.chunk0[a]) * GR_CHUNK;
    const int64_t hi = lo + GR_CHUNK < rb ? lo + GR_CHUNK : rb;
    const char* s = (i >= 0 && i < g.src_rows) ? g.src[a] + i * rb : nullptr;
    char* d = g.dst[a] + (int64_t)r * rb;
    if (g.width[a] == 16) gr_copy<gr_u32x4>(s, d, lo, hi);
    else if (g.width[a] == 8) gr_copy<gr_u32x2>(s, d, lo, hi);
    else gr_copy<uint32_t>(s, d, lo, hi);
  }
}

}  // namespace mimrl

using namespace mimrl;

extern "C" int mimrl_op_gather_rows(void* stream, int n_arrays, const void* const* src, void* const* dst, const int64_t* row_bytes,
                                    int64_t src_rows, const int32_t* idx, int rows, int max_workgroups) {
  if (n_arrays < 1 || n_arrays > 4) return set_error(MIMRL_ERR_ARG, "gather_rows: %d arrays outside [1, 4]", n_arrays);
  if (!src || !dst || !row_bytes || !idx) return set_error(MIMRL_ERR_ARG, "gather_rows: null argument");
  if (rows < 1) return set_error(MIMRL_ERR_ARG, "gather_rows: %d destination rows (need at least 1)", rows);
  if (src_rows < 0 || max_workgroups < 0) return set_error(MIMRL_ERR_ARG, "gather_rows: negative src_rows / max_workgroups");
  GatherRowsArgs g;
  g.n = n_arrays; g.rows = rows; g.src_rows = src_rows; g.idx = idx;
  g.chunk0[0] = 0;
  for (int a = 0; a < 4; ++a) {
    if (a >= n_arrays) { g.src[a] = nullptr; g.dst[a] = nullptr; g.row_bytes[a] = 0; g.width[a] = 4; g.chunk0[a + 1] = g.chunk0[a]; continue; }
    if (!src[a] || !dst[a]) return set_error(MIMRL_ERR_ARG, "gather_rows: array %d has a null pointer", a);
    const int64_t rb = row_bytes[a];
    if (rb < 4 || rb % 4 != 0) return set_error(MIMRL_ERR_ARG, "gather_rows: row_bytes[%d] = %lld is not a positive multiple of 4", a, (long long)rb);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(src[a]) | reinterpret_cast<uintptr_t>(dst[a]) | (uintptr_t)rb;
    if (bits % 4 != 0) return set_error(MIMRL_ERR_ARG, "gather_rows: array %d is not 4-byte aligned", a);
    const int64_t chunks = (rb + GR_CHUNK - 1) / GR_CHUNK;
    if (chunks > (1 << 20)) return set_error(MIMRL_ERR_ARG, "gather_rows: row_bytes[%d] = %lld is too long", a, (long long)rb);
    g.src[a] = static_cast<const char*>(src[a]); g.dst[a] = static_cast<char*>(dst[a]); g.row_bytes[a] = rb;
    g.width[a] = bits % 16 == 0 ? 16 : bits % 8 == 0 ? 8 : 4;      // every row then starts on that boundary in both arrays
    g.chunk0[a + 1] = g.chunk0[a] + (int)chunks;
  }
  const int64_t items = (int64_t)rows * g.chunk0[n_arrays];
  int64_t grid = max_workgroups > 0 ? max_workgroups : 8 * (int64_t)device_cus();
  if (grid > items) grid = items;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)grid), dim3(GR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), g);
  LAUNCH_CHECK();
  return MIMRL_OK;
}
