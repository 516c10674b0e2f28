// libfsi_kernel_shim.so — test-only entry points over single fsi::launch_* calls of libvaspfsi.so (tests/kernel_shim.py).
//
// Not loaded by the product, bench.py or smoke().  Every entry point takes host arrays and does nothing but: allocate device
// buffers and upload the inputs (outputs are uploaded too, so that a sentinel the caller placed shows whether the kernel wrote
// where it must not), run ONE launch function on a private stream, synchronise, check hipGetLastError, copy the outputs back.
// A null host pointer is passed to the launch as a null device pointer.  Status: 0 = ok, nonzero = HIP error
// (shim_last_error() says which), or the launch function's own nonzero status passed through (LAUNCH_REFUSED of fsi_kernels.hpp:
// the launch refused its arguments and launched nothing; the outputs are still copied back).
//
// Vectors of the node-block sweeps are float4 per node (component 3 is padding), as the preconditioner holds them.
#include "fsi_host.hpp"
#include "fsi_kernels.hpp"

#include <cstring>

using namespace fsi;

namespace {

thread_local std::string g_err;

struct Call {
  struct Back { void* h; const void* d; size_t bytes; };
  hipStream_t st = nullptr;
  hipError_t e = hipSuccess;
  std::vector<void*> bufs;
  std::vector<Back> backs;
  Call() { note(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }
  ~Call() {
    for (void* p : bufs) (void)hipFree(p);
    if (st) (void)hipStreamDestroy(st);
  }
  void note(hipError_t x) { if (e == hipSuccess && x != hipSuccess) e = x; }
  bool ok() const { return e == hipSuccess; }
  // device copy of count host elements (at least 16 bytes are allocated, so that an empty array is still a non-null pointer)
  template <class T>
  T* in(const T* h, size_t count) {
    if (!h || !ok()) return nullptr;
    void* d = nullptr;
    const size_t bytes = count * sizeof(T);
    note(hipMalloc(&d, bytes < 16 ? 16 : bytes));
    if (!ok()) return nullptr;
    bufs.push_back(d);
    if (bytes) note(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return static_cast<T*>(d);
  }
  // as in(), and copied back into h after the launch
  template <class T>
  T* io(T* h, size_t count) {
    T* d = in<T>(h, count);
    if (d) backs.push_back({h, d, count * sizeof(T)});
    return d;
  }
  int finish(const char* what) {
    if (ok()) note(hipGetLastError());
    if (ok()) note(hipStreamSynchronize(st));
    if (ok()) note(hipGetLastError());
    for (const Back& b : backs)
      if (ok() && b.bytes) note(hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost));
    if (ok()) return 0;
    g_err = std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")";
    return 1;
  }
};

#define SHIM_RUN(call, what, ...) \
  do {                            \
    if (call.ok()) __VA_ARGS__;   \
    return call.finish(what);     \
  } while (0)
// as SHIM_RUN, for launch functions that return a status of their own
#define SHIM_RUN_STATUS(call, what, ...)                                                   \
  do {                                                                                     \
    int st_ = 0;                                                                           \
    if (call.ok()) st_ = __VA_ARGS__;                                                      \
    if (const int e_ = call.finish(what)) return e_;                                       \
    if (st_) g_err = std::string(what) + ": refused its arguments (status " + std::to_string(st_) + "), nothing launched"; \
    return st_;                                                                            \
  } while (0)

}  // namespace

extern "C" {

const char* shim_last_error() { return g_err.c_str(); }

// ---- fsi_gcr.hip ------------------------------------------------------------------------------------------------------
// Q: m columns of ldq entries (float if fp32, else double); out: nout >= m + 2 doubles
int shim_gcr_dots(int fp32, const void* Q, int64_t ldq, int64_t n, int m, const double* w, const double* r, double* out,
                  int64_t nout) {
  Call c;
  const size_t qb = (size_t)ldq * (size_t)m * (fp32 ? 4 : 8);
  const void* dQ = c.in(static_cast<const char*>(Q), qb);
  const double* dw = c.in(w, (size_t)n);
  const double* dr = c.in(r, (size_t)n);
  std::vector<double> hs((size_t)(m + 2) * 1024 + 16);      // the partial sums: (m + 2) x at most 1024 row parts
  double* scratch = c.in(hs.data(), hs.size());
  double* dout = c.io(out, (size_t)nout);
  SHIM_RUN(c, "launch_gcr_dots", launch_gcr_dots(c.st, fp32 != 0, dQ, ldq, n, m, dw, dr, scratch, dout));
}
// w (n) in place; out2: nout >= 2 doubles
int shim_gcr_axpy(int fp32, const void* Q, int64_t ldq, int64_t n, int m, const double* h, double* w, const double* r,
                  double* out2, int64_t nout) {
  Call c;
  const void* dQ = c.in(static_cast<const char*>(Q), (size_t)ldq * (size_t)m * (fp32 ? 4 : 8));
  const double* dh = c.in(h, (size_t)(m > 0 ? m : 0));
  double* dw = c.io(w, (size_t)n);
  const double* dr = c.in(r, (size_t)n);
  std::vector<double> hs(2 * 2048 + 16);
  double* scratch = c.in(hs.data(), hs.size());
  double* dout = c.io(out2, (size_t)nout);
  SHIM_RUN(c, "launch_gcr_axpy", launch_gcr_axpy(c.st, fp32 != 0, dQ, ldq, n, m, dh, dw, dr, scratch, dout));
}
// Q: ncols columns of ldq (in place), Z: ncols columns of ldz (in place), r, qd (n, in place); out1: nout >= 1
int shim_gcr_update(int fp32, void* Q, int64_t ldq, double* Z, int64_t ldz, int ncols, int slot, int64_t n, const double* w,
                    const double* z, double inv_wn, double alpha, double* r, double* qd, double* out1, int64_t nout) {
  Call c;
  void* dQ = c.io(static_cast<char*>(Q), (size_t)ldq * (size_t)ncols * (fp32 ? 4 : 8));
  double* dZ = c.io(Z, (size_t)ldz * (size_t)ncols);
  const double* dw = c.in(w, (size_t)n);
  const double* dz = c.in(z, (size_t)n);
  double* dr = c.io(r, (size_t)n);
  double* dqd = c.io(qd, (size_t)n);
  std::vector<double> hs(2048 + 16);
  double* scratch = c.in(hs.data(), hs.size());
  double* dout = c.io(out1, (size_t)nout);
  SHIM_RUN(c, "launch_gcr_update",
           launch_gcr_update(c.st, fp32 != 0, dQ, ldq, dZ, ldz, slot, n, dw, dz, inv_wn, alpha, dr, dqd, scratch, dout));
}
int shim_gcr_flush_width(int knew) { return gcr_flush_width(knew); }
// Z: ncols columns of ldz (in place); y: m; cn: gcr_flush_width(knew) x m; slots: knew; x: n (in place)
int shim_gcr_flush(double* Z, int64_t ldz, int ncols, int64_t n, int m, const double* y, const double* cn, const int32_t* slots,
                   int knew, double* x) {
  Call c;
  double* dZ = c.io(Z, (size_t)ldz * (size_t)ncols);
  const double* dy = c.in(y, (size_t)m);
  const double* dcn = c.in(cn, (size_t)gcr_flush_width(knew) * (size_t)m);
  const int32_t* ds = c.in(slots, (size_t)knew);
  double* dx = c.io(x, (size_t)n);
  SHIM_RUN(c, "launch_gcr_flush", launch_gcr_flush(c.st, dZ, ldz, n, m, dy, dcn, ds, knew, dx));
}

// ---- fsi_solver.hip: deterministic reductions ---------------------------------------------------------------------------
int shim_dot(const double* x, const double* y, int64_t n, double* out) {
  Call c;
  const double* dx = c.in(x, (size_t)n);
  const double* dy = c.in(y, (size_t)n);
  std::vector<double> hs(4096 + 16);
  double* scratch = c.in(hs.data(), hs.size());
  double* dout = c.io(out, 2);
  SHIM_RUN(c, "launch_dot", launch_dot(c.st, dx, dy, n, scratch, dout));
}
// x: nx entries, the sum reads x[first + i * stride] for i < n
int shim_hashed_sum(const double* x, int64_t nx, int64_t first, int64_t stride, int64_t n, double* out) {
  Call c;
  const double* dx = c.in(x, (size_t)nx);
  std::vector<double> hs(4096 + 16);
  double* scratch = c.in(hs.data(), hs.size());
  double* dout = c.io(out, 2);
  SHIM_RUN(c, "launch_hashed_sum", launch_hashed_sum(c.st, dx, first, stride, n, scratch, dout));
}

// ---- fsi_block.hip: displacement / velocity node blocks ------------------------------------------------------------------
// Graph: nadj_ptr [N2 + 1], nadj [pairs]; vals: nv per pair; tiles of tn nodes: tile_uptr [ntiles + 1], ulist, ploc [pairs].
// rowflag: 3 N2 (may be null where the launch allows it); dinv and the vectors: 4 N2 floats.
static int64_t tiles_of(int64_t N2, int tn) { return (N2 + tn - 1) / tn; }
int shim_spmv_sc_f32(int64_t N2, const int64_t* nadj_ptr, const int32_t* nadj, const float* chat, const uint8_t* rowflag,
                     const float* x, float* y) {
  Call c;
  const int64_t np = nadj_ptr[N2];
  const int64_t* dp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const float* dc = c.in(chat, (size_t)np);
  const uint8_t* df = c.in(rowflag, (size_t)(3 * N2));
  const float* dx = c.in(x, (size_t)(4 * N2));
  float* dy = c.io(y, (size_t)(4 * N2));
  SHIM_RUN(c, "launch_spmv_sc_f32", launch_spmv_sc_f32(c.st, N2, dp, dn, dc, df, dx, dy));
}
int shim_sweep_sc_f32(int64_t N2, const int64_t* nadj_ptr, const int32_t* nadj, const float* chat, const uint8_t* rowflag,
                      float c1, float c2, const float* din, float* dout, float* x, float* r) {
  Call c;
  const int64_t np = nadj_ptr[N2];
  const int64_t* dp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const float* dc = c.in(chat, (size_t)np);
  const uint8_t* df = c.in(rowflag, (size_t)(3 * N2));
  float* ddi = c.io(const_cast<float*>(din), (size_t)(4 * N2));
  float* ddo = c.io(dout, (size_t)(4 * N2));
  float* dx = c.io(x, (size_t)(4 * N2));
  float* dr = c.io(r, (size_t)(4 * N2));
  SHIM_RUN(c, "launch_sweep_sc_f32", launch_sweep_sc_f32(c.st, N2, dp, dn, dc, df, c1, c2, ddi, ddo, dx, dr));
}
int shim_spmv_db_f32(int64_t N2, const int64_t* nadj_ptr, const int32_t* nadj, const float* db, const float* x, float* y) {
  Call c;
  const int64_t np = nadj_ptr[N2];
  const int64_t* dp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const float* dd = c.in(db, (size_t)(3 * np));
  const float* dx = c.in(x, (size_t)(4 * N2));
  float* dy = c.io(y, (size_t)(4 * N2));
  SHIM_RUN(c, "launch_spmv_db_f32", launch_spmv_db_f32(c.st, N2, dp, dn, dd, dx, dy));
}
int shim_spmv_tiled_f32(int nv, int tn, int64_t N2, int max_nu, const int64_t* nadj_ptr, const float* vals, const uint16_t* ploc,
                        const int64_t* tile_uptr, const int32_t* ulist, const uint8_t* rowflag, const float* x, float* y) {
  Call c;
  const int64_t np = nadj_ptr[N2], nt = tiles_of(N2, tn);
  const int64_t* dp = c.in(nadj_ptr, (size_t)N2 + 1);
  const float* dv = c.in(vals, (size_t)(nv * np));
  const uint16_t* dl = c.in(ploc, (size_t)np);
  const int64_t* du = c.in(tile_uptr, (size_t)nt + 1);
  const int32_t* dul = c.in(ulist, (size_t)tile_uptr[nt]);
  const uint8_t* df = c.in(rowflag, (size_t)(3 * N2));
  const float* dx = c.in(x, (size_t)(4 * N2));
  float* dy = c.io(y, (size_t)(4 * N2));
  SHIM_RUN(c, "launch_spmv_tiled_f32", launch_spmv_tiled_f32(c.st, nv, tn, N2, max_nu, dp, dv, dl, du, dul, df, dx, dy));
}
int shim_sweep_tiled_f32(int nv, int tn, int64_t N2, int max_nu, const int64_t* nadj_ptr, const float* vals, const uint16_t* ploc,
                         const int64_t* tile_uptr, const int32_t* ulist, const uint8_t* rowflag, const float* dinv, float c1,
                         float c2, float* din, float* dout, float* x, float* r) {
  Call c;
  const int64_t np = nadj_ptr[N2], nt = tiles_of(N2, tn);
  const int64_t* dp = c.in(nadj_ptr, (size_t)N2 + 1);
  const float* dv = c.in(vals, (size_t)(nv * np));
  const uint16_t* dl = c.in(ploc, (size_t)np);
  const int64_t* du = c.in(tile_uptr, (size_t)nt + 1);
  const int32_t* dul = c.in(ulist, (size_t)tile_uptr[nt]);
  const uint8_t* df = c.in(rowflag, (size_t)(3 * N2));
  const float* ddv = c.in(dinv, (size_t)(4 * N2));
  float* ddi = c.io(din, (size_t)(4 * N2));
  float* ddo = c.io(dout, (size_t)(4 * N2));
  float* dx = c.io(x, (size_t)(4 * N2));
  float* dr = c.io(r, (size_t)(4 * N2));
  SHIM_RUN(c, "launch_sweep_tiled_f32",
           launch_sweep_tiled_f32(c.st, nv, tn, N2, max_nu, dp, dv, dl, du, dul, df, ddv, c1, c2, ddi, ddo, dx, dr));
}
// rec: the records of launch_pack_h1 (nv = 1: 1 word per pair) / launch_pack_h3 (nv = 3: 2 words per pair)
int shim_sweep_tiled_h(int nv, int tn, int64_t N2, int max_nu, const int64_t* nadj_ptr, const uint32_t* rec, const int64_t* tile_uptr,
                       const int32_t* ulist, const uint8_t* rowflag, const float* dinv, float c1, float c2, float* din, float* dout,
                       float* x, float* r) {
  Call c;
  const int64_t np = nadj_ptr[N2], nt = tiles_of(N2, tn);
  const int64_t* dp = c.in(nadj_ptr, (size_t)N2 + 1);
  const uint32_t* drec = c.in(rec, (size_t)((nv == 1 ? 1 : 2) * np));
  const int64_t* du = c.in(tile_uptr, (size_t)nt + 1);
  const int32_t* dul = c.in(ulist, (size_t)tile_uptr[nt]);
  const uint8_t* df = c.in(rowflag, (size_t)(3 * N2));
  const float* ddv = c.in(dinv, (size_t)(4 * N2));
  float* ddi = c.io(din, (size_t)(4 * N2));
  float* ddo = c.io(dout, (size_t)(4 * N2));
  float* dx = c.io(x, (size_t)(4 * N2));
  float* dr = c.io(r, (size_t)(4 * N2));
  SHIM_RUN(c, "launch_sweep_tiled_h",
           launch_sweep_tiled_h(c.st, nv, tn, N2, max_nu, dp, drec, du, dul, df, ddv, c1, c2, ddi, ddo, dx, dr));
}
// FP16 records.  h1: rec[e] = half(v[e]) | loc[e] << 16.  h3: rec[2e] = half(v[3e]) | half(v[3e+1]) << 16,
// rec[2e+1] = half(v[3e+2]) | loc[e] << 16.  sb: per 3x3 block six words (a0 a1)(a2 a3)(a4 a5)(a6 a7)(a8 0)(column).
// half() is the device's float -> _Float16 conversion (round to nearest even).
int shim_pack_h1(int64_t n, const float* v, const uint16_t* loc, uint32_t* rec) {
  Call c;
  const float* dv = c.in(v, (size_t)n);
  const uint16_t* dl = c.in(loc, (size_t)n);
  uint32_t* drec = c.io(rec, (size_t)n);
  SHIM_RUN(c, "launch_pack_h1", launch_pack_h1(c.st, n, dv, dl, drec));
}
int shim_pack_h3(int64_t n, const float* v, const uint16_t* loc, uint32_t* rec) {
  Call c;
  const float* dv = c.in(v, (size_t)(3 * n));
  const uint16_t* dl = c.in(loc, (size_t)n);
  uint32_t* drec = c.io(rec, (size_t)(2 * n));
  SHIM_RUN(c, "launch_pack_h3", launch_pack_h3(c.st, n, dv, dl, drec));
}
int shim_pack_sb(int64_t nb, const float* v, const int32_t* col, uint32_t* rec) {
  Call c;
  const float* dv = c.in(v, (size_t)(9 * nb));
  const int32_t* dc = c.in(col, (size_t)nb);
  uint32_t* drec = c.io(rec, (size_t)(6 * nb));
  SHIM_RUN(c, "launch_pack_sb", launch_pack_sb(c.st, nb, dv, dc, drec));
}
// n floats; dinv may not be null
int shim_cheb_init_f32(int64_t n, const float* rhs, const float* dinv, float inv_theta, float* x, float* r, float* d) {
  Call c;
  const float* drhs = c.in(rhs, (size_t)n);
  const float* ddv = c.in(dinv, (size_t)n);
  float* dx = c.io(x, (size_t)n);
  float* dr = c.io(r, (size_t)n);
  float* dd = c.io(d, (size_t)n);
  SHIM_RUN(c, "launch_cheb_init_f32", launch_cheb_init_f32(c.st, n, drhs, ddv, inv_theta, dx, dr, dd));
}
int shim_cheb_step_f32(int64_t n, const float* t, const float* dinv, float c1, float c2, float* x, float* r, float* d) {
  Call c;
  const float* dt = c.in(t, (size_t)n);
  const float* ddv = c.in(dinv, (size_t)n);
  float* dx = c.io(x, (size_t)n);
  float* dr = c.io(r, (size_t)n);
  float* dd = c.io(d, (size_t)n);
  SHIM_RUN(c, "launch_cheb_step_f32", launch_cheb_step_f32(c.st, n, dt, ddv, c1, c2, dx, dr, dd));
}

// ---- fsi_block.hip: solid block (3x3 block CSR over nS nodes; vals 9 per block, row-major; binv12: 3 rows of 4 per node) -----
int shim_spmv_sb(int64_t nS, const int64_t* sb_ptr, const int32_t* sb_col, const float* vals, const float* x, float* y) {
  Call c;
  const int64_t nb = sb_ptr[nS];
  const int64_t* dp = c.in(sb_ptr, (size_t)nS + 1);
  const int32_t* dc = c.in(sb_col, (size_t)nb);
  const float* dv = c.in(vals, (size_t)(9 * nb));
  const float* dx = c.in(x, (size_t)(4 * nS));
  float* dy = c.io(y, (size_t)(4 * nS));
  SHIM_RUN(c, "launch_spmv_sb", launch_spmv_sb(c.st, nS, dp, dc, dv, dx, dy));
}
int shim_sweep_sb_b3(int64_t nS, const int64_t* sb_ptr, const int32_t* sb_col, const float* vals, const float* binv12, float c1,
                     float c2, float* din, float* dout, float* x, float* r, int level) {
  Call c;
  const int64_t nb = sb_ptr[nS];
  const int64_t* dp = c.in(sb_ptr, (size_t)nS + 1);
  const int32_t* dc = c.in(sb_col, (size_t)nb);
  const float* dv = c.in(vals, (size_t)(9 * nb));
  const float* dbi = c.in(binv12, (size_t)(12 * nS));
  float* ddi = c.io(din, (size_t)(4 * nS));
  float* ddo = c.io(dout, (size_t)(4 * nS));
  float* dx = c.io(x, (size_t)(4 * nS));
  float* dr = c.io(r, (size_t)(4 * nS));
  SHIM_RUN(c, "launch_sweep_sb_b3", launch_sweep_sb_b3(c.st, nS, dp, dc, dv, dbi, c1, c2, ddi, ddo, dx, dr, level));
}
int shim_sweep_sb_h(int64_t nS, const int64_t* sb_ptr, const uint32_t* rec, const float* binv12, float c1, float c2, float* din,
                    float* dout, float* x, float* r) {
  Call c;
  const int64_t nb = sb_ptr[nS];
  const int64_t* dp = c.in(sb_ptr, (size_t)nS + 1);
  const uint32_t* drec = c.in(rec, (size_t)(6 * nb));
  const float* dbi = c.in(binv12, (size_t)(12 * nS));
  float* ddi = c.io(din, (size_t)(4 * nS));
  float* ddo = c.io(dout, (size_t)(4 * nS));
  float* dx = c.io(x, (size_t)(4 * nS));
  float* dr = c.io(r, (size_t)(4 * nS));
  SHIM_RUN(c, "launch_sweep_sb_h", launch_sweep_sb_h(c.st, nS, dp, drec, dbi, c1, c2, ddi, ddo, dx, dr));
}
int shim_cheb_init_b3(int64_t nS, const float* rhs, const float* binv12, float inv_theta, float* x, float* r, float* d) {
  Call c;
  const float* drhs = c.in(rhs, (size_t)(4 * nS));
  const float* dbi = c.in(binv12, (size_t)(12 * nS));
  float* dx = c.io(x, (size_t)(4 * nS));
  float* dr = c.io(r, (size_t)(4 * nS));
  float* dd = c.io(d, (size_t)(4 * nS));
  SHIM_RUN(c, "launch_cheb_init_b3", launch_cheb_init_b3(c.st, nS, drhs, dbi, inv_theta, dx, dr, dd));
}
int shim_cheb_step_b3(int64_t nS, const float* t, const float* binv12, float c1, float c2, float* x, float* r, float* d) {
  Call c;
  const float* dt = c.in(t, (size_t)(4 * nS));
  const float* dbi = c.in(binv12, (size_t)(12 * nS));
  float* dx = c.io(x, (size_t)(4 * nS));
  float* dr = c.io(r, (size_t)(4 * nS));
  float* dd = c.io(d, (size_t)(4 * nS));
  SHIM_RUN(c, "launch_cheb_step_b3", launch_cheb_step_b3(c.st, nS, dt, dbi, c1, c2, dx, dr, dd));
}

// ---- fsi_block.hip: Schur sweeps (CSR over n rows; FP64 vectors of n) -----------------------------------------------------
int shim_sweep_csr_f64(int64_t n, const int64_t* rowptr, const int32_t* cols, const double* vals, const int64_t* diagpos, double c1,
                       double c2, double* din, double* dout, double* x, double* r) {
  Call c;
  const int64_t nnz = rowptr[n];
  const int64_t* dp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)nnz);
  const double* dv = c.in(vals, (size_t)nnz);
  const int64_t* dg = c.in(diagpos, (size_t)n);
  double* ddi = c.io(din, (size_t)n);
  double* ddo = c.io(dout, (size_t)n);
  double* dx = c.io(x, (size_t)n);
  double* dr = c.io(r, (size_t)n);
  SHIM_RUN(c, "launch_sweep_csr_f64", launch_sweep_csr_f64(c.st, n, dp, dc, dv, dg, c1, c2, ddi, ddo, dx, dr));
}
int shim_sweep_csr_mixed(int64_t n, const int64_t* rowptr, const int32_t* cols, const float* vals, const int64_t* diagpos,
                         const double* dvals, double c1, double c2, double* din, double* dout, double* x, double* r) {
  Call c;
  const int64_t nnz = rowptr[n];
  const int64_t* dp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)nnz);
  const float* dv = c.in(vals, (size_t)nnz);
  const int64_t* dg = c.in(diagpos, (size_t)n);
  const double* ddv = c.in(dvals, (size_t)nnz);
  double* ddi = c.io(din, (size_t)n);
  double* ddo = c.io(dout, (size_t)n);
  double* dx = c.io(x, (size_t)n);
  double* dr = c.io(r, (size_t)n);
  SHIM_RUN(c, "launch_sweep_csr_mixed", launch_sweep_csr_mixed(c.st, n, dp, dc, dv, dg, ddv, c1, c2, ddi, ddo, dx, dr));
}
// rec: launch_pack_h1 records of the values with tile-local columns; tiles of tile_rows rows: tile_uptr, ulist
int shim_sweep_schur_tiled(int tile_rows, int64_t n, int max_nu, const int64_t* rowptr, const uint32_t* rec, const int64_t* tile_uptr,
                           const int32_t* ulist, const double* dinv, double c1, double c2, double* din, double* dout, double* x,
                           double* r) {
  Call c;
  const int64_t nnz = rowptr[n], nt = (n + tile_rows - 1) / tile_rows;
  const int64_t* dp = c.in(rowptr, (size_t)n + 1);
  const uint32_t* drec = c.in(rec, (size_t)nnz);
  const int64_t* du = c.in(tile_uptr, (size_t)nt + 1);
  const int32_t* dul = c.in(ulist, (size_t)tile_uptr[nt]);
  const double* ddv = c.in(dinv, (size_t)n);
  double* ddi = c.io(din, (size_t)n);
  double* ddo = c.io(dout, (size_t)n);
  double* dx = c.io(x, (size_t)n);
  double* dr = c.io(r, (size_t)n);
  SHIM_RUN(c, "launch_sweep_schur_tiled",
           launch_sweep_schur_tiled(c.st, tile_rows, n, max_nu, dp, drec, du, dul, ddv, c1, c2, ddi, ddo, dx, dr));
}

int shim_tile_limit() { return tile_limit(); }

// ---- fsi_solver.hip: the monolithic matrix's structure and products -----------------------------------------------------------
// Node graph: nadj_ptr [N2 + 1], nadj [npairs = nadj_ptr[N2]]; pressure graph: padj_ptr [N2 + 1], padj [padj_ptr[N2]]; vrank [V];
// rows: 6 N2 node rows then V pressure rows, rowptr [6 N2 + V + 1], nnz = rowptr[6 N2 + V].  x and y: 6 N2 + V entries.
int shim_expand_cols(int64_t N2, int64_t V, const int64_t* nadj_ptr, const int32_t* nadj, const int64_t* padj_ptr, const int32_t* padj,
                     const int32_t* vrank, const int64_t* rowptr, int32_t* cols, int64_t* diagpos) {
  Call c;
  const int64_t n = 6 * N2 + V;
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)nadj_ptr[N2]);
  const int64_t* dpp = c.in(padj_ptr, (size_t)N2 + 1);
  const int32_t* dpa = c.in(padj, (size_t)padj_ptr[N2]);
  const int32_t* dvr = c.in(vrank, (size_t)V);
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  int32_t* dc = c.io(cols, (size_t)rowptr[n]);
  int64_t* ddp = c.io(diagpos, (size_t)n);
  SHIM_RUN(c, "launch_expand_cols", launch_expand_cols(c.st, N2, V, dnp, dn, dpp, dpa, dvr, drp, dc, ddp));
}
// generic CSR over n rows; x: nx entries
int shim_spmv(int64_t n, const int64_t* rowptr, const int32_t* cols, const double* vals, const double* x, int64_t nx, double* y, int tag) {
  Call c;
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n]);
  const double* dv = c.in(vals, (size_t)rowptr[n]);
  const double* dx = c.in(x, (size_t)nx);
  double* dy = c.io(y, (size_t)n);
  SHIM_RUN(c, "launch_spmv", launch_spmv(c.st, n, drp, dc, dv, dx, dy, tag));
}
// vrank, nadj_ptr, nadj may each be null (npairs: the length of nadj, and ad64 holds 6 npairs)
int shim_spmv_node6(int64_t N2, int64_t V, const int64_t* rowptr, const int32_t* cols, const double* vals, const int32_t* vrank,
                    const int64_t* nadj_ptr, const int32_t* nadj, int64_t npairs, const double* x, double* y, const double* ad64) {
  Call c;
  const int64_t n = 6 * N2 + V;
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n]);
  const double* dv = c.in(vals, (size_t)rowptr[n]);
  const PRowGraph g{c.in(vrank, (size_t)V), c.in(nadj_ptr, (size_t)N2 + 1), c.in(nadj, (size_t)npairs)};
  const double* dx = c.in(x, (size_t)n);
  double* dy = c.io(y, (size_t)n);
  const double* dad = c.in(ad64, (size_t)(6 * npairs));
  SHIM_RUN_STATUS(c, "launch_spmv_node6", launch_spmv_node6(c.st, N2, V, drp, dc, dv, g, dx, dy, dad));
}
// node rows only: rowptr [6 N2 + 1], A [rowptr[6 N2]]; ad64 / ad32 [6 nadj_ptr[N2]] (ad32 may be null); flag [1]
int shim_drows_extract(int64_t N2, const int64_t* rowptr, const double* A, const int64_t* nadj_ptr, double* ad64, float* ad32,
                       int32_t* flag) {
  Call c;
  const int64_t npairs = nadj_ptr[N2];
  const int64_t* drp = c.in(rowptr, (size_t)(6 * N2) + 1);
  const double* dA = c.in(A, (size_t)rowptr[6 * N2]);
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  double* d64 = c.io(ad64, (size_t)(6 * npairs));
  float* d32 = c.io(ad32, (size_t)(6 * npairs));
  int32_t* df = c.io(flag, 1);
  SHIM_RUN(c, "launch_drows_extract", launch_drows_extract(c.st, N2, drp, dA, dnp, d64, d32, df));
}
// p32 [N2 + 1] (entries, six value rows per node block); cols32 [p32[N2] / 6]
int shim_pad_cols32(int64_t N2, const int64_t* rowptr, const int32_t* cols, const int64_t* p32, int32_t* cols32) {
  Call c;
  const int64_t* drp = c.in(rowptr, (size_t)(6 * N2) + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[6 * N2]);
  const int64_t* dp = c.in(p32, (size_t)N2 + 1);
  int32_t* dc32 = c.io(cols32, (size_t)(p32[N2] / 6));
  SHIM_RUN(c, "launch_pad_cols32", launch_pad_cols32(c.st, N2, drp, dc, dp, dc32));
}
// A [rowptr[6 N2 + V]]; A32 [n32]
int shim_pad_vals32(int64_t N2, int64_t V, const int64_t* rowptr, const double* A, const int64_t* p32, int64_t ptail, int64_t nnz_tail,
                    int64_t tail_src, float* A32, int64_t n32, int v_rows_only) {
  Call c;
  const int64_t* drp = c.in(rowptr, (size_t)(6 * N2 + V) + 1);
  const double* dA = c.in(A, (size_t)rowptr[6 * N2 + V]);
  const int64_t* dp = c.in(p32, (size_t)N2 + 1);
  float* d32 = c.io(A32, (size_t)n32);
  SHIM_RUN(c, "launch_pad_vals32", launch_pad_vals32(c.st, N2, V, drp, dA, dp, ptail, nnz_tail, tail_src, d32, v_rows_only != 0));
}
// vals [n32]; the pressure rows' values at vals + tail_shift + rowptr[row]; ad32 [6 npairs] or null
int shim_spmv_node6p(int64_t N2, int64_t V, const int64_t* p32, const int32_t* cols32, const float* vals, int64_t n32, const int64_t* rowptr,
                     const int32_t* cols, int64_t tail_shift, const int32_t* vrank, const int64_t* nadj_ptr, const int32_t* nadj, int64_t npairs,
                     const double* x, double* y, const float* ad32) {
  Call c;
  const int64_t n = 6 * N2 + V;
  const int64_t* dp = c.in(p32, (size_t)N2 + 1);
  const int32_t* dc32 = c.in(cols32, (size_t)(p32[N2] / 6));
  const float* dv = c.in(vals, (size_t)n32);
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n]);
  const PRowGraph g{c.in(vrank, (size_t)V), c.in(nadj_ptr, (size_t)N2 + 1), c.in(nadj, (size_t)npairs)};
  const double* dx = c.in(x, (size_t)n);
  double* dy = c.io(y, (size_t)n);
  const float* dad = c.in(ad32, (size_t)(6 * npairs));
  SHIM_RUN_STATUS(c, "launch_spmv_node6p", launch_spmv_node6p(c.st, N2, V, dp, dc32, dv, drp, dc, tail_shift, g, dx, dy, dad));
}
// n rows; A (in place), Apre [rowptr[n]]; bc [nbc] (may repeat); rowscale, bcmask [n]
int shim_matrix_finish(int64_t n, const int64_t* rowptr, const int64_t* diagpos, double* A, const double* Apre, const int32_t* bc,
                       int64_t nbc, double* rowscale, int32_t* bcmask) {
  Call c;
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int64_t* ddp = c.in(diagpos, (size_t)n);
  double* dA = c.io(A, (size_t)rowptr[n]);
  const double* dpre = c.in(Apre, (size_t)rowptr[n]);
  const int32_t* dbc = c.in(bc, (size_t)nbc);
  double* drs = c.io(rowscale, (size_t)n);
  int32_t* dbm = c.io(bcmask, (size_t)n);
  SHIM_RUN(c, "launch_matrix_finish", launch_matrix_finish(c.st, n, drp, ddp, dA, dpre, dbc, nbc, drs, dbm));
}

// ---- a live context's preconditioner arrays (FsiCtx of fsi_context.hpp, as the library was compiled) -----------------------
// shim_ctx_info: N2, V, nS, sb_nblocks, tiled, tile_nodes, tile_max_nu, schur_tiled, schur_tile, s_tile_max_nu, sweeps_fp16,
// a32_ptail, a32_tail_src, a32_tail_nnz, op32_ok, kry_fp32, drows_ok
int shim_ctx_info(const FsiCtx* ctx, int64_t* out, int nout) {
  const int64_t v[] = {ctx->N2, ctx->V, ctx->nS, ctx->sb_nblocks, ctx->tiled, ctx->tile_nodes, ctx->tile_max_nu,
                       ctx->schur_tiled, ctx->schur_tile, ctx->s_tile_max_nu, ctx->sweeps_fp16,
                       ctx->a32_ptail, ctx->a32_tail_src, ctx->a32_tail_nnz, ctx->op32_ok, ctx->kry_fp32, ctx->drows_ok};
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < nout && i < k; ++i) out[i] = v[i];
  return k;
}
// the factor of the solid columns' displacement entries folded into the velocity block (Avv~ = Avv + ktheta Avd, k_extract_blocks)
double shim_ctx_ktheta(const FsiCtx* ctx) { return ctx->scheme.k * ctx->scheme.th0; }
// Copies the named device array into host (when host is not null); *count / *elem: its length and element size.
// Status 2: no such name.
int shim_ctx_array(const FsiCtx* ctx, const char* name, void* host, int64_t* count, int* elem) {
  struct Entry { const char* name; const void* p; size_t n, sz; };
#define E(f) Entry{#f, ctx->f.p, ctx->f.n, sizeof(*ctx->f.p)}
  const Entry table[] = {E(nadj_ptr), E(nadj),        E(dd_chat), E(dd_rowflag), E(dd_rec),      E(tile_ploc),   E(tile_uptr),
                         E(tile_ulist), E(vv_db32),   E(vv_rec),  E(sb_ptr),     E(sb_col),      E(sb_vals),     E(sb_rec),
                         E(sb_binv12),  E(s_rowptr),  E(s_cols),  E(s_diagpos),  E(s_vals),      E(s_vals32),    E(s_rec),
                         E(s_ploc),     E(s_tile_uptr), E(s_tile_ulist), E(s_dinv), E(dd_db),    E(rowscale),    E(snode),
                         E(solver2user), E(node_solid), E(rowptr),    E(cols),        E(diagpos),     E(A),           E(vrank),
                         E(padj_ptr),   E(padj),      E(A32),     E(a32_ptr),    E(a32_cols),    E(Ad64),        E(Ad32)};
#undef E
  for (const Entry& t : table) {
    if (std::strcmp(t.name, name) != 0) continue;
    *count = (int64_t)t.n;
    *elem = (int)t.sz;
    if (host && t.n) {
      const hipError_t e = hipMemcpy(host, t.p, t.n * t.sz, hipMemcpyDeviceToHost);
      if (e != hipSuccess) { g_err = std::string("shim_ctx_array ") + name + ": " + hipGetErrorName(e); return 1; }
    }
    return 0;
  }
  g_err = std::string("shim_ctx_array: unknown array ") + name;
  return 2;
}

// y = the context's monolithic product of x (solver ordering, row-equilibrated: no permutation, no un-scaling), through
// fsi::host::spmv(ctx, x, y, working); x, y [ndof].  counters [2]: what the call added to op32_products and drows_products.
// Status: 0, 1 = HIP error, else the FSI_ERR_* of host::spmv (ctx->err in shim_last_error()).
int shim_ctx_spmv(FsiCtx* ctx, int working, const double* x, double* y, int64_t* counters) {
  Call c;
  const int64_t n = ctx->ndof;
  const double* dx = c.in(x, (size_t)n);
  double* dy = c.io(y, (size_t)n);
  if (c.ok()) c.note(hipSetDevice(ctx->device));
  const int64_t op0 = ctx->op32_products, dr0 = ctx->drows_products;
  int rc = 0;
  if (c.ok()) {
    rc = fsi::host::spmv(ctx, dx, dy, working != 0);
    c.note(hipStreamSynchronize(ctx->stream));
  }
  counters[0] = ctx->op32_products - op0;
  counters[1] = ctx->drows_products - dr0;
  if (const int e = c.finish("host::spmv")) return e;
  if (rc) g_err = "host::spmv: " + ctx->err;
  return rc;
}

}  // extern "C"
