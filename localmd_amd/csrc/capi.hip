// The context of libpmd_hip.so: the route switches it reads when it is created, its life cycle and the event profile.
// Every other entry point of include/pmd_hip.h is defined in the file that implements it.
#include "pmd_internal.h"

// ---------------------------------------------------------------- route switches ----------
// Every PMD_* variable the library reads, in the order of DESIGN.md section 6a.  A row with accepted values maps each text
// to the field's value; a row without any takes a number.  Unset, or a text that is not accepted: the default.
namespace {
struct route_value { const char* text; int value; };
struct route_row {
  const char* name;
  int pmd_routes::*field;
  double pmd_routes::*real_field;    // set instead of `field` for the one fractional knob
  double dflt;
  route_value accepted[4];           // ends at the first NULL text
};
const route_row ROUTE_TABLE[] = {
    {"PMD_SYEVD", &pmd_routes::syevd, nullptr, PMD_SYEVD_AUTO,
     {{"f64", PMD_SYEVD_F64}, {"rocsolver", PMD_SYEVD_ROCSOLVER}, {"own", PMD_SYEVD_OWN}, {"twostage", PMD_SYEVD_TWOSTAGE}}},
    {"PMD_APPLY_Q", &pmd_routes::apply_q_rocsolver, nullptr, 0, {{"rocsolver", 1}}},
    {"PMD_SYR2K", &pmd_routes::syr2k_rocblas, nullptr, 0, {{"rocblas", 1}}},
    {"PMD_CHOLESKY", &pmd_routes::cholesky_rocsolver, nullptr, 0, {{"rocsolver", 1}}},
    {"PMD_CHOL_CHAIN", &pmd_routes::chol_chain_rocblas, nullptr, 0, {{"rocblas", 1}}},
    {"PMD_SYTRD_ADVANCE", &pmd_routes::sytrd_advance_old, nullptr, 0, {{"old", 1}}},
    {"PMD_GEMM_SPLIT", &pmd_routes::gemm_split, nullptr, 1, {{"0", 0}}},
    {"PMD_GEMM_SPLIT_MIN_GFLOP", nullptr, &pmd_routes::gemm_split_min_gflop, 100.0, {}},
    {"PMD_GEMM_SPLIT_MIN_DIM", &pmd_routes::gemm_split_min_dim, nullptr, 256, {}},
    {"PMD_GEMM_SPLITK", &pmd_routes::gemm_splitk, nullptr, 1, {{"0", 0}}},
    {"PMD_GEMM_KCHUNK", &pmd_routes::gemm_kchunk, nullptr, -1, {}},
    {"PMD_F16X2_MTGM", &pmd_routes::f16x2_mtgm, nullptr, 6, {{"0", 0}}},
    {"PMD_GRAM_APPLY_MFMA", &pmd_routes::gram_apply_mfma, nullptr, 1, {{"0", 0}}},
    {"PMD_GRAM_MFMA", &pmd_routes::gram_mfma, nullptr, 1, {{"0", 0}}},
    {"PMD_ROWMIX_MFMA", &pmd_routes::rowmix_mfma, nullptr, -1, {{"0", 0}, {"16", 16}, {"64", 64}}},
    {"PMD_ATX_DMA", &pmd_routes::atx_dma, nullptr, 1, {{"0", 0}}},
    {"PMD_TILE_WHITEN", &pmd_routes::tile_whiten_eig, nullptr, 0, {{"eig", 1}}},
    {"PMD_WIDE_EIG", &pmd_routes::wide_eig_syevd, nullptr, 0, {{"syevd", 1}}},
    {"PMD_SMALL_EIG", &pmd_routes::small_eig_rocsolver, nullptr, 0, {{"rocsolver", 1}}},
};

void pmd_routes_from_env(pmd_routes* r) {
  for (const route_row& row : ROUTE_TABLE) {
    const char* text = getenv(row.name);
    double v = row.dflt;
    if (text && !row.accepted[0].text) v = atof(text);
    for (const route_value& a : row.accepted)
      if (text && a.text && !strcmp(text, a.text)) v = a.value;
    if (row.real_field) r->*row.real_field = v;
    else r->*row.field = (int)v;
  }
}
}  // namespace

extern "C" {

int pmd_version(void) { return 1; }

int pmd_ctx_create(int device, void* hip_stream, pmd_ctx** out) {
  if (!out) return PMD_ERR_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return PMD_ERR_HIP;
  if (hipSetDevice(device) != hipSuccess) return PMD_ERR_HIP;
  pmd_ctx* ctx = new pmd_ctx();
  ctx->device = device;
  ctx->stream = (hipStream_t)hip_stream;
  pmd_routes_from_env(&ctx->routes);
  if (rocblas_create_handle(&ctx->blas) != rocblas_status_success) { delete ctx; return PMD_ERR_BLAS; }
  rocblas_set_stream(ctx->blas, ctx->stream);
  rocblas_set_pointer_mode(ctx->blas, rocblas_pointer_mode_host);
  if (pmd_init_tables(ctx) != PMD_OK) { rocblas_destroy_handle(ctx->blas); delete ctx; return PMD_ERR_HIP; }
  *out = ctx;
  return PMD_OK;
}

int pmd_ctx_destroy(pmd_ctx* ctx) {
  CTX_CHECK(ctx);
  hipSetDevice(ctx->device);
  if (ctx->comm) pmd_comm_destroy(ctx);
  if (ctx->tables) hipFree(ctx->tables);
  if (ctx->scratch) hipFree(ctx->scratch);
  if (ctx->scratch2) hipFree(ctx->scratch2);
  if (ctx->split_ws) hipFree(ctx->split_ws);
  pmd_f16x2_destroy(ctx);
  if (ctx->blas) rocblas_destroy_handle(ctx->blas);
  delete ctx;
  return PMD_OK;
}

int pmd_ctx_set_null_cutoff(pmd_ctx* ctx, float rel_cutoff) {
  CTX_CHECK(ctx);
  ctx->null_cutoff = rel_cutoff;
  return PMD_OK;
}

int pmd_ctx_set_stream(pmd_ctx* ctx, void* hip_stream) {
  CTX_CHECK(ctx);
  ctx->stream = (hipStream_t)hip_stream;
  rocblas_set_stream(ctx->blas, ctx->stream);
  return PMD_OK;
}

int pmd_ctx_sync(pmd_ctx* ctx) {
  CTX_CHECK(ctx);
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PMD_OK;
}

const char* pmd_last_error(pmd_ctx* ctx) { return ctx ? ctx->err : "null context"; }

int pmd_profile_enable(pmd_ctx* ctx, int on) {
  CTX_CHECK(ctx);
  for (auto& r : ctx->recs) { (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop); }
  ctx->recs.clear();
  ctx->profile = on != 0;
  return PMD_OK;
}

// Sum of the event-timed durations of every launch group called `name` since the last
// pmd_profile_enable (synchronises the stream).  total_ms/count may be NULL.
int pmd_profile_query(pmd_ctx* ctx, const char* name, double* total_ms, int* count) {
  CTX_CHECK(ctx);
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double tot = 0.0;
  int n = 0;
  for (auto& r : ctx->recs) {
    if (strcmp(r.name, name) != 0) continue;
    float ms = 0.f;
    PMD_HIP(ctx, hipEventElapsedTime(&ms, r.start, r.stop));
    tot += ms;
    n++;
  }
  if (total_ms) *total_ms = tot;
  if (count) *count = n;
  return PMD_OK;
}

// Names seen so far, '\n'-separated, written into buf (truncated to cap-1 characters).
int pmd_profile_names(pmd_ctx* ctx, char* buf, int cap) {
  CTX_CHECK(ctx);
  if (!buf || cap < 1) return PMD_ERR_ARG;
  buf[0] = 0;
  std::vector<const char*> seen;
  for (auto& r : ctx->recs) {
    bool dup = false;
    for (auto s : seen) dup = dup || strcmp(s, r.name) == 0;
    if (dup) continue;
    seen.push_back(r.name);
    if ((int)(strlen(buf) + strlen(r.name) + 2) >= cap) break;
    strcat(buf, r.name);
    strcat(buf, "\n");
  }
  return PMD_OK;
}

}  // extern "C"
