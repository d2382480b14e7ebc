// Internal header of libpmd_hip.so (gfx950 only).  Public C ABI: include/pmd_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>
#include <vector>

#include "../../include/pmd_hip.h"   // enum pmd_elem

#define PMD_OK 0
#define PMD_ERR_HIP -1
#define PMD_ERR_ARG -2
#define PMD_ERR_WORKSPACE -3
#define PMD_ERR_BLAS -4
#define PMD_ERR_UNSUPPORTED -5

#define PMD_RPAD 64          // component rows of every per-tile [comp][x] array
#define PMD_LD_SLACK 64      // extra floats at the end of every time-contiguous row

// random streams (oracle/philox.py holds the same numbers)
#define PMD_STREAM_BG_OMEGA 1
#define PMD_STREAM_SIM_NOISE 2
#define PMD_STREAM_SIM_OMEGA 3
#define PMD_STREAM_TILE_OMEGA 4
#define PMD_STREAM_PRUNE 5

struct pmd_prof_rec {
  const char* name;
  hipEvent_t start, stop;
};

// Route switches: A/B comparators and library-routine fallbacks selected by PMD_* environment variables.  The table in
// capi.hip is the list of them (one row per variable: field, default, accepted values).  They are read ONCE, when a
// context is created, and are fixed for that context; a value outside a row's accepted set means the default.
enum { PMD_SYEVD_AUTO = 0, PMD_SYEVD_F64, PMD_SYEVD_ROCSOLVER, PMD_SYEVD_OWN, PMD_SYEVD_TWOSTAGE };
struct pmd_routes {
  int syevd;                         // PMD_SYEVD: one of PMD_SYEVD_* (sytrd.hip)
  int apply_q_rocsolver;             // PMD_APPLY_Q=rocsolver: sormtr in place of the blocked back-transformation
  int syr2k_rocblas;                 // PMD_SYR2K=rocblas: ssyr2k in place of the rank-2k kernel of the tridiagonalisation
  int cholesky_rocsolver;            // PMD_CHOLESKY=rocsolver: spotrf in place of the blocked factorisation (and no fp64 form of small orders)
  int chol_chain_rocblas;            // PMD_CHOL_CHAIN=rocblas: strtri + sgemm per panel in place of chol_panel_kernel
  int sytrd_advance_old;             // PMD_SYTRD_ADVANCE=old: 64 positions x 4 parts per workgroup
  int gemm_split;                    // PMD_GEMM_SPLIT: 1 (default) = large fp32 products as fp16-piece products (gemm_f16x2.hip); 0: rocBLAS sgemm only
  double gemm_split_min_gflop;       // PMD_GEMM_SPLIT_MIN_GFLOP: ... for products of at least this many GFLOP
  int gemm_split_min_dim;            // PMD_GEMM_SPLIT_MIN_DIM: ... and no dimension below this
  int gemm_splitk;                   // PMD_GEMM_SPLITK: 1 (default) = strided-batched split-K sgemm for few output tiles and a long k
  int gemm_kchunk;                   // PMD_GEMM_KCHUNK: length of one fp32 accumulation chain; -1 (default) = by k, 0 = whole k
  int f16x2_mtgm;                    // PMD_F16X2_MTGM: 6 (default) = M^T G M as concatenated fp16-piece products; 0: sgemm
  int gram_apply_mfma;               // PMD_GRAM_APPLY_MFMA: 1 (default); 0: the scalar gram_apply_kernel
  int gram_mfma;                     // PMD_GRAM_MFMA: 1 (default); 0: the scalar tile_gram_kernel
  int rowmix_mfma;                   // PMD_ROWMIX_MFMA: -1 (default) = by shape; 0: scalar kernels; 16 / 64: that many positions per wave
  int atx_dma;                       // PMD_ATX_DMA: 1 (default) = LDS-DMA staged tile_atx for d in (256, 400]; 0: the plain variant
  int tile_whiten_eig;               // PMD_TILE_WHITEN=eig: eigenvector form of the two pure orthonormalisation steps
  int wide_eig_syevd;                // PMD_WIDE_EIG=syevd: rocSOLVER's batched divide-and-conquer solver in place of dsyevj
  int small_eig_rocsolver;           // PMD_SMALL_EIG=rocsolver: the tile eigenproblems through the wide (rocSOLVER) path
};

struct pmd_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  rocblas_handle blas = nullptr;
  float* tables = nullptr;           // device: Hann window + FFT twiddles, see prep.hip
  char err[512] = "";
  void* scratch = nullptr;           // library-owned device scratch of the eigensolver (sytrd.hip)
  size_t scratch_bytes = 0;
  void* scratch2 = nullptr;          // library-owned device scratch of the fp64 eigenvector refinement (sytrd.hip)
  size_t scratch2_bytes = 0;
  pmd_routes routes;                 // the PMD_* route switches, as the environment had them when the context was created
  void* f16x2 = nullptr;             // state of gemm_f16x2.hip (hipBLASLt handle, plans), created on first use
  void* split_ws = nullptr;          // library-owned device scratch of the split products (fp16 pieces, split-K partial sums)
  size_t split_ws_bytes = 0;
  void* comm = nullptr;              // RCCL communicator (pmd_comm_init), NULL without one
  int comm_rank = 0, comm_world = 0;
  float null_cutoff = -1.f;          // < 0: keep every direction with lambda != 0, scaled by 1/sqrt(|lambda|) (decomposition.py:984-996);
                                     // >= 0: keep lambda > null_cutoff * lambda_max only (pmd_ctx_set_null_cutoff)
  bool profile = false;              // pmd_profile_enable: HIP events around every kernel group
  std::vector<pmd_prof_rec> recs;
};

// RAII: records a start/stop event pair on the context's stream around one launcher call
struct pmd_prof_scope {
  pmd_ctx* ctx;
  pmd_prof_rec rec;
  bool on;
  pmd_prof_scope(pmd_ctx* c, const char* name) : ctx(c), on(c && c->profile) {
    if (!on) return;
    rec.name = name;
    if (hipEventCreate(&rec.start) != hipSuccess || hipEventCreate(&rec.stop) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(rec.start, ctx->stream);
  }
  ~pmd_prof_scope() {
    if (!on) return;
    (void)hipEventRecord(rec.stop, ctx->stream);
    ctx->recs.push_back(rec);
  }
};

static inline int pmd_fail(pmd_ctx* ctx, int code, const char* what, const char* detail) {
  if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s: %s", what, detail ? detail : "");
  return code;
}

#define PMD_HIP(ctx, call)                                                        \
  do {                                                                            \
    hipError_t e__ = (call);                                                      \
    if (e__ != hipSuccess) return pmd_fail(ctx, PMD_ERR_HIP, #call, hipGetErrorString(e__)); \
  } while (0)

#define PMD_LAUNCH_CHECK(ctx, name)                                               \
  do {                                                                            \
    hipError_t e__ = hipGetLastError();                                           \
    if (e__ != hipSuccess) return pmd_fail(ctx, PMD_ERR_HIP, name, hipGetErrorString(e__)); \
  } while (0)

// first line of every entry point that takes a context
#define CTX_CHECK(ctx) \
  if (!(ctx)) return PMD_ERR_ARG;

// passes a failed library call's return code on to the caller
#define RUN(call)                    \
  do {                               \
    int rc__ = (call);               \
    if (rc__ != PMD_OK) return rc__; \
  } while (0)

static inline long pmd_round_up(long x, long m) { return (x + m - 1) / m * m; }

// XCD-aware tile order.  Workgroups go to the 8 XCDs round-robin by linear workgroup id, and each XCD has its
// own L2.  Tiles overlap their neighbours by 50 %, so instead of dealing tiles 0,1,2,... across the XCDs, every
// XCD gets a contiguous run of the tile list and walks it in order: neighbouring tiles then run on the same XCD
// at about the same time and the second reader of a shared pixel row hits that XCD's L2.
// For a grid whose x dimension counts tiles: returns the tile of this workgroup (a bijection on [0, gridDim.x)).
#ifdef __HIPCC__
__device__ __forceinline__ int pmd_xcd_tile() {
  const int n = (int)gridDim.x, x = (int)blockIdx.x;
  if (n < 64) return x;
  const int row = (int)(blockIdx.y + gridDim.y * blockIdx.z);
  const int s = (int)(((long)n * row) & 7);      // XCD of the first workgroup of this grid row
  const int c = (x + s) & 7;                     // XCD of this workgroup
  const int x0 = (c - s) & 7;                    // first x of the row that lands on XCD c
  const int m = (x - x0) >> 3;                   // how many earlier workgroups of the row that XCD got
  // tiles before XCD c's run: XCD c' owns the x values x0' = (c' - s) & 7, x0' + 8, ... below n
  int off = 0;
  for (int cp = 0; cp < c; ++cp) {
    const int x0p = (cp - s) & 7;
    off += (n - x0p + 7) >> 3;
  }
  return off + m;
}

// value -> output element: fp32 as is; 16-bit integers round half to even, saturate, NaN -> 0 (export.quantize on the
// host).  The one conversion of pmd_group_expand, pmd_shift_apply and pmd_warp_apply.
template <typename O>
__device__ __forceinline__ O pmd_quant(float v) {
  if constexpr (sizeof(O) == 4) {
    return v;
  } else {
    const float mn = std::is_signed<O>::value ? -32768.f : 0.f;
    const float mx = std::is_signed<O>::value ? 32767.f : 65535.f;
    if (v != v) return (O)0;
    const float r = fminf(fmaxf(rintf(v), mn), mx);
    return (O)(int)r;
  }
}
#endif

// ---- element types and strided images (host side of the launchers) --------------------------------------------------
static inline bool pmd_bad_elem(int e) { return e != PMD_ELEM_F32 && e != PMD_ELEM_U16 && e != PMD_ELEM_I16; }
static inline size_t pmd_elem_size(int e) { return e == PMD_ELEM_F32 ? 4 : 2; }

// f(pmd_elem_tag<T>{}) with T the C type of ``elem`` (checked with pmd_bad_elem before); in f, ``typename
// decltype(tag)::type`` is T
template <typename T>
struct pmd_elem_tag {
  using type = T;
};
template <typename F>
static inline void pmd_with_elem(int elem, F&& f) {
  switch (elem) {
    case PMD_ELEM_F32: f(pmd_elem_tag<float>{}); break;
    case PMD_ELEM_U16: f(pmd_elem_tag<uint16_t>{}); break;
    default: f(pmd_elem_tag<int16_t>{}); break;
  }
}

// n frames of d1 x d2 elements at the given strides (in elements): a row stride shorter than a row, or a frame stride
// shorter than a frame
static inline bool pmd_short_strides(long frame_stride, long row_stride, int d1, int d2) {
  return row_stride < d2 || frame_stride < (long)(d1 - 1) * row_stride + d2;
}

// whether the byte ranges of two such images, first element to last, intersect (n >= 1)
static inline bool pmd_images_overlap(const void* X, int elem, long frame_stride, long row_stride, const void* out,
                                      int out_elem, long out_frame_stride, long out_row_stride, int n, int d1, int d2) {
  const uintptr_t xa = (uintptr_t)X, oa = (uintptr_t)out;
  const uintptr_t xe = xa + ((size_t)(n - 1) * frame_stride + (size_t)(d1 - 1) * row_stride + d2) * pmd_elem_size(elem);
  const uintptr_t oe =
      oa + ((size_t)(n - 1) * out_frame_stride + (size_t)(d1 - 1) * out_row_stride + d2) * pmd_elem_size(out_elem);
  return xa < oe && oa < xe;
}

// carve a caller-provided workspace
struct pmd_arena {
  char* base;
  size_t size;
  size_t used;
  bool overflow;
  pmd_arena(void* p, size_t n) : base((char*)p), size(n), used(0), overflow(false) {}
  void* take(size_t bytes) {
    size_t off = (used + 255) & ~size_t(255);
    used = off + bytes;
    if (base == nullptr || used > size) {
      overflow = true;
      return nullptr;
    }
    return base + off;
  }
  template <typename T>
  T* take_n(size_t n) { return (T*)take(n * sizeof(T)); }
};

// padded pixel count of a tile and the tile_atx kernel variant that serves it
struct pmd_dvariant {
  int kjw;   // 16-row groups per wave
  int ks;    // K split (waves = 4*ks)
  int tc;    // frames per chunk
  int dpad;  // = 16*kjw*ks
};
static inline bool pmd_pick_dvariant(int d, pmd_dvariant* v) {
  static const pmd_dvariant table[] = {
      {16, 1, 32, 256}, {25, 1, 32, 400}, {32, 1, 32, 512},
      {25, 2, 32, 800}, {32, 2, 32, 1024}, {25, 4, 16, 1600}};
  for (const auto& t : table)
    if (d <= t.dpad) { *v = t; return true; }
  return false;
}
