// mimrl_op_gather_packed: the batch upload of a PACKED dataset (data.Packed: the frames of all samples back to back, no padding).  Row r of
// dst[a] is frames[a] frames of frame_bytes[a] bytes: the first min(length[a][i], frames[a]) of them come from src[a] at frame start[a][i],
// i = idx[r]; the rest of the row is zero -- the padded batch the engine's input sets hold, written by ONE launch for up to four arrays.  An
// array without start / length is dense (the labels): row i is copied whole, as mimrl_op_gather_rows does.
//
// Work item = (destination row r, chunk c) exactly as in gather_rows.hip: GP_CHUNK bytes of a DESTINATION row, the chunks of the arrays of
// one row numbered one array after the other, the grid striding over the items (any max_workgroups writes the same bytes).  idx[r] and the
// start / length of sample i in every packed array are wave-uniform loads, made only after i passed its range check.  frame_bytes is a
// multiple of the lane width, so the boundary between frames and padding falls between two lanes' vectors: a lane loads or stores zero,
// never both halves; a chunk that lies wholly in the padding issues no load.  A sample whose index, start or length cannot be honoured in
// ANY array is never used as an address: its destination row becomes NaN in every array (gather_rows' convention).  Plain vector loads and
// stores, no LDS, no accumulation (det.hip: nothing to flush behind it -- it runs on the upload stream, where a flush must not run).
#include "common.h"

namespace mimrl {

constexpr int GP_THREADS = 256;
constexpr int GP_CHUNK = 16384;      // bytes of a destination row per work item: 4 x 16-byte vectors per lane
constexpr int GP_UNROLL = 4;         // loads in flight per lane

struct GatherPackedArgs {
  const char* src[4];
  char* dst[4];
  const int64_t* start[4];           // nullptr: a dense array
  const int32_t* length[4];
  int64_t frame_bytes[4];
  int64_t row_bytes[4];              // frames * frame_bytes
  int64_t src_frames[4];
  int32_t frames[4];
  int32_t chunk0[5];                 // first chunk number of array a within a row; chunk0[n] = chunks per row
  int32_t width[4];                  // bytes per lane: 16, 8 or 4
  int32_t n;
  int32_t rows;
  int64_t src_rows;
  const int32_t* idx;
};

typedef uint32_t gp_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t gp_u32x2 __attribute__((ext_vector_type(2)));

template <class V> __device__ __forceinline__ V gp_splat(uint32_t x);
template <> __device__ __forceinline__ uint32_t gp_splat<uint32_t>(uint32_t x) { return x; }
template <> __device__ __forceinline__ gp_u32x2 gp_splat<gp_u32x2>(uint32_t x) { return gp_u32x2{x, x}; }
template <> __device__ __forceinline__ gp_u32x4 gp_splat<gp_u32x4>(uint32_t x) { return gp_u32x4{x, x, x, x}; }

// bytes [lo, hi) of one destination row d: those below `valid` come from s (the sample's first frame), the others are `fill`; s, d, lo, hi
// and valid are aligned to sizeof(V)
template <class V>
__device__ __forceinline__ void gp_copy(const char* s, char* d, int64_t lo, int64_t hi, int64_t valid, uint32_t fill) {
  constexpr int64_t W = sizeof(V);
  for (int64_t b = lo + (int64_t)threadIdx.x * W; b < hi; b += (int64_t)GP_THREADS * W * GP_UNROLL) {
    V v[GP_UNROLL];
#pragma unroll
    for (int k = 0; k < GP_UNROLL; ++k) {
      const int64_t o = b + (int64_t)k * GP_THREADS * W;
      v[k] = gp_splat<V>(fill);
      if (o < valid) v[k] = __builtin_nontemporal_load(reinterpret_cast<const V*>(s + o));
    }
#pragma unroll
    for (int k = 0; k < GP_UNROLL; ++k) {
      const int64_t o = b + (int64_t)k * GP_THREADS * W;
      if (o < hi) *reinterpret_cast<V*>(d + o) = v[k];
    }
  }
}

__global__ void __launch_bounds__(GP_THREADS) gather_packed_kernel(GatherPackedArgs g) {
  const int per_row = g.chunk0[g.n];
  const int64_t items = (int64_t)g.rows * per_row;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int r = (int)(item / per_row);
    const int c = (int)(item - (int64_t)r * per_row);
    int a = 0;
    while (a + 1 < g.n && c >= g.chunk0[a + 1]) ++a;
    const int64_t i = g.idx[r];
    bool ok = i >= 0 && i < g.src_rows;
    int64_t st = 0, ln = 0;          // of array a
    if (ok) {
      for (int b = 0; b < g.n; ++b) {
        if (!g.start[b]) continue;
        const int64_t sb = g.start[b][i];
        const int64_t lb = g.length[b][i];
        if (sb < 0 || lb < 0 || sb > g.src_frames[b] - lb) ok = false;
        if (b == a) { st = sb; ln = lb; }
      }
    }
    const int64_t rb = g.row_bytes[a];
    const int64_t lo = (int64_t)(c - g.chunk0[a]) * GP_CHUNK;
    const int64_t hi = lo + GP_CHUNK < rb ? lo + GP_CHUNK : rb;
    int64_t valid = 0;               // bytes of the row that come from the source
    const char* s = nullptr;
    if (ok) {
      if (g.start[a]) {
        if (ln > g.frames[a]) ln = g.frames[a];
        valid = ln * g.frame_bytes[a];
        s = g.src[a] + st * g.frame_bytes[a];
      } else {
        valid = rb;
        s = g.src[a] + i * rb;
      }
    }
    const uint32_t fill = ok ? 0u : 0x7fc00000u;
    char* d = g.dst[a] + (int64_t)r * rb;
    if (g.width[a] == 16) gp_copy<gp_u32x4>(s, d, lo, hi, valid, fill);
    else if (g.width[a] == 8) gp_copy<gp_u32x2>(s, d, lo, hi, valid, fill);
    else gp_copy<uint32_t>(s, d, lo, hi, valid, fill);
  }
}

}  // namespace mimrl

using namespace mimrl;

extern "C" int mimrl_op_gather_packed(void* stream, int n_arrays, const void* const* src, void* const* dst, const int64_t* frame_bytes,
                                      const int32_t* frames, const int64_t* const* start, const int32_t* const* length,
                                      const int64_t* src_frames, int64_t src_rows, const int32_t* idx, int rows, int max_workgroups) {
  if (n_arrays < 1 || n_arrays > 4) return set_error(MIMRL_ERR_ARG, "gather_packed: %d arrays outside [1, 4]", n_arrays);
  if (!src || !dst || !frame_bytes || !frames || !start || !length || !src_frames || !idx) return set_error(MIMRL_ERR_ARG, "gather_packed: null argument");
  if (rows < 1) return set_error(MIMRL_ERR_ARG, "gather_packed: %d destination rows (need at least 1)", rows);
  if (src_rows < 0 || max_workgroups < 0) return set_error(MIMRL_ERR_ARG, "gather_packed: negative src_rows / max_workgroups");
  GatherPackedArgs g;
  g.n = n_arrays; g.rows = rows; g.src_rows = src_rows; g.idx = idx;
  g.chunk0[0] = 0;
  for (int a = 0; a < 4; ++a) {
    if (a >= n_arrays) {
      g.src[a] = nullptr; g.dst[a] = nullptr; g.start[a] = nullptr; g.length[a] = nullptr; g.frame_bytes[a] = 0; g.row_bytes[a] = 0;
      g.src_frames[a] = 0; g.frames[a] = 0; g.width[a] = 4; g.chunk0[a + 1] = g.chunk0[a];
      continue;
    }
    if (!src[a] || !dst[a]) return set_error(MIMRL_ERR_ARG, "gather_packed: array %d has a null pointer", a);
    if ((start[a] == nullptr) != (length[a] == nullptr))
      return set_error(MIMRL_ERR_ARG, "gather_packed: array %d has only one of start / length (both, or neither for dense rows)", a);
    const int64_t fb = frame_bytes[a];
    if (fb < 4 || fb % 4 != 0) return set_error(MIMRL_ERR_ARG, "gather_packed: frame_bytes[%d] = %lld is not a positive multiple of 4", a, (long long)fb);
    if (frames[a] < 1) return set_error(MIMRL_ERR_ARG, "gather_packed: frames[%d] = %d (need at least 1)", a, (int)frames[a]);
    if (start[a] && src_frames[a] < 0) return set_error(MIMRL_ERR_ARG, "gather_packed: src_frames[%d] = %lld is negative", a, (long long)src_frames[a]);
    if (start[a] && (reinterpret_cast<uintptr_t>(start[a]) % 8 != 0 || reinterpret_cast<uintptr_t>(length[a]) % 4 != 0))
      return set_error(MIMRL_ERR_ARG, "gather_packed: start / length of array %d are not aligned to their element size", a);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(src[a]) | reinterpret_cast<uintptr_t>(dst[a]) | (uintptr_t)fb;
    if (bits % 4 != 0) return set_error(MIMRL_ERR_ARG, "gather_packed: array %d is not 4-byte aligned", a);
    if (fb > ((int64_t)1 << 34) / frames[a]) return set_error(MIMRL_ERR_ARG, "gather_packed: a row of array %d (%d frames of %lld bytes) is too long", a, (int)frames[a], (long long)fb);
    const int64_t rb = fb * frames[a];
    const int64_t chunks = (rb + GP_CHUNK - 1) / GP_CHUNK;
    g.src[a] = static_cast<const char*>(src[a]); g.dst[a] = static_cast<char*>(dst[a]);
    g.start[a] = start[a]; g.length[a] = length[a];
    g.frame_bytes[a] = fb; g.row_bytes[a] = rb; g.src_frames[a] = src_frames[a]; g.frames[a] = frames[a];
    g.width[a] = bits % 16 == 0 ? 16 : bits % 8 == 0 ? 8 : 4;      // every frame, and so every row, then starts on that boundary in both arrays
    g.chunk0[a + 1] = g.chunk0[a] + (int)chunks;
  }
  const int64_t items = (int64_t)rows * g.chunk0[n_arrays];
  int64_t grid = max_workgroups > 0 ? max_workgroups : 8 * (int64_t)device_cus();
  if (grid > items) grid = items;
  hipLaunchKernelGGL(gather_packed_kernel, dim3((unsigned)grid), dim3(GP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), g);
  LAUNCH_CHECK();
  return MIMRL_OK;
}
