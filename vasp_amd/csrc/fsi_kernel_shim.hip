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
//
// A live context is read through shim_ctx_info / shim_ctx_coarse / shim_ctx_array (device arrays by name; `blk`, the work vectors
// of one preconditioner application, and the two cycles' coarse work areas `sbmg_work` / `mg_work` among them) and
// shim_ctx_apply_info (what precondition_block branches on and the sweep counts it takes): tests/block_apply.py.  Its recycled
// GCR is read and run through shim_ctx_krylov_info / shim_ctx_krylov_columns / shim_ctx_solve_gcr / shim_ctx_precondition
// (whole host functions of fsi_krylov.hip and fsi_precond.hip on the context's own stream): tests/gcr_solve.py.
#include "fsi_cheb.hpp"
#include "fsi_host.hpp"
#include "fsi_kernels.hpp"
#include "fsi_room.hpp"

#include <cmath>
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
// the two above over m columns of which the leading md hold data (launch_gcr_dots_lead / launch_gcr_axpy_lead)
int shim_gcr_dots_lead(int fp32, const void* Q, int64_t ldq, int64_t n, int m, int md, const double* w, const double* r, double* out,
                       int64_t nout) {
  Call c;
  const void* dQ = c.in(static_cast<const char*>(Q), (size_t)ldq * (size_t)m * (fp32 ? 4 : 8));
  const double* dw = c.in(w, (size_t)n);
  const double* dr = c.in(r, (size_t)n);
  std::vector<double> hs((size_t)(m + 2) * 1024 + 16);
  double* scratch = c.in(hs.data(), hs.size());
  double* dout = c.io(out, (size_t)nout);
  SHIM_RUN(c, "launch_gcr_dots_lead", launch_gcr_dots_lead(c.st, fp32 != 0, dQ, ldq, n, m, md, dw, dr, scratch, dout));
}
int shim_gcr_axpy_lead(int fp32, const void* Q, int64_t ldq, int64_t n, int m, int md, const double* h, double* w, const double* r,
                       double* out2, int64_t nout) {
  Call c;
  const void* dQ = c.in(static_cast<const char*>(Q), (size_t)ldq * (size_t)m * (fp32 ? 4 : 8));
  const double* dh = c.in(h, (size_t)(m > 0 ? m : 0));
  double* dw = c.io(w, (size_t)n);
  const double* dr = c.in(r, (size_t)n);
  std::vector<double> hs(2 * 2048 + 16);
  double* scratch = c.in(hs.data(), hs.size());
  double* dout = c.io(out2, (size_t)nout);
  SHIM_RUN(c, "launch_gcr_axpy_lead", launch_gcr_axpy_lead(c.st, fp32 != 0, dQ, ldq, n, m, md, dh, dw, dr, scratch, dout));
}
// Q: ncols columns of ldq (in place), Z: ncols columns of ldz (in place), r, qd (n, in place; qd may be null); out1: nout >= 1
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
// what the four tiled sweep entries share on the device: the graph's row pointers, the tiles, rowflag, dinv and the four vectors
struct TiledSweepArgs {
  const int64_t *dp, *du;
  const int32_t* dul;
  const uint8_t* df;
  const float* ddv;
  float *ddi, *ddo, *dx, *dr;
  TiledSweepArgs(Call& c, int tn, int64_t N2, const int64_t* nadj_ptr, const int64_t* tile_uptr, const int32_t* ulist,
                 const uint8_t* rowflag, const float* dinv, float* din, float* dout, float* x, float* r) {
    const int64_t nt = tiles_of(N2, tn);
    dp = c.in(nadj_ptr, (size_t)N2 + 1);
    du = c.in(tile_uptr, (size_t)nt + 1);
    dul = c.in(ulist, (size_t)tile_uptr[nt]);
    df = c.in(rowflag, (size_t)(3 * N2));
    ddv = c.in(dinv, (size_t)(4 * N2));
    ddi = c.io(din, (size_t)(4 * N2));
    ddo = c.io(dout, (size_t)(4 * N2));
    dx = c.io(x, (size_t)(4 * N2));
    dr = c.io(r, (size_t)(4 * N2));
  }
};
int shim_sweep_tiled_f32(int nv, int tn, int64_t N2, int max_nu, const int64_t* nadj_ptr, const float* vals, const uint16_t* ploc,
                         const int64_t* tile_uptr, const int32_t* ulist, const uint8_t* rowflag, const float* dinv, float c1,
                         float c2, float* din, float* dout, float* x, float* r) {
  Call c;
  const int64_t np = nadj_ptr[N2];
  const float* dv = c.in(vals, (size_t)(nv * np));
  const uint16_t* dl = c.in(ploc, (size_t)np);
  const TiledSweepArgs a(c, tn, N2, nadj_ptr, tile_uptr, ulist, rowflag, dinv, din, dout, x, r);
  SHIM_RUN(c, "launch_sweep_tiled_f32",
           launch_sweep_tiled_f32(c.st, nv, tn, N2, max_nu, a.dp, dv, dl, a.du, a.dul, a.df, a.ddv, c1, c2, a.ddi, a.ddo, a.dx, a.dr));
}
// rec: the records of launch_pack_h1 (nv = 1: 1 word per pair) / launch_pack_h3 (nv = 3: 2 words per pair)
int shim_sweep_tiled_h(int nv, int tn, int64_t N2, int max_nu, const int64_t* nadj_ptr, const uint32_t* rec, const int64_t* tile_uptr,
                       const int32_t* ulist, const uint8_t* rowflag, const float* dinv, float c1, float c2, float* din, float* dout,
                       float* x, float* r) {
  Call c;
  const uint32_t* drec = c.in(rec, (size_t)((nv == 1 ? 1 : 2) * nadj_ptr[N2]));
  const TiledSweepArgs a(c, tn, N2, nadj_ptr, tile_uptr, ulist, rowflag, dinv, din, dout, x, r);
  SHIM_RUN(c, "launch_sweep_tiled_h",
           launch_sweep_tiled_h(c.st, nv, tn, N2, max_nu, a.dp, drec, a.du, a.dul, a.df, a.ddv, c1, c2, a.ddi, a.ddo, a.dx, a.dr));
}
// rec: the records of launch_pack_f3 (4 words per pair)
int shim_sweep_tiled_r3(int tn, int64_t N2, int max_nu, const int64_t* nadj_ptr, const uint32_t* rec, const int64_t* tile_uptr,
                        const int32_t* ulist, const uint8_t* rowflag, const float* dinv, float c1, float c2, float* din, float* dout,
                        float* x, float* r) {
  Call c;
  const uint32_t* drec = c.in(rec, (size_t)(4 * nadj_ptr[N2]));
  const TiledSweepArgs a(c, tn, N2, nadj_ptr, tile_uptr, ulist, rowflag, dinv, din, dout, x, r);
  SHIM_RUN(c, "launch_sweep_tiled_r3",
           launch_sweep_tiled_r3(c.st, tn, N2, max_nu, a.dp, drec, a.du, a.dul, a.df, a.ddv, c1, c2, a.ddi, a.ddo, a.dx, a.dr));
}
// the one-ratio sweep (as shim_sweep_tiled_f32 with nv = 1) with two rows ahead in flight
int shim_sweep_tiled_a1(int tn, int64_t N2, int max_nu, const int64_t* nadj_ptr, const float* vals, const uint16_t* ploc,
                        const int64_t* tile_uptr, const int32_t* ulist, const uint8_t* rowflag, const float* dinv, float c1, float c2,
                        float* din, float* dout, float* x, float* r) {
  Call c;
  const int64_t np = nadj_ptr[N2];
  const float* dv = c.in(vals, (size_t)np);
  const uint16_t* dl = c.in(ploc, (size_t)np);
  const TiledSweepArgs a(c, tn, N2, nadj_ptr, tile_uptr, ulist, rowflag, dinv, din, dout, x, r);
  SHIM_RUN(c, "launch_sweep_tiled_a1",
           launch_sweep_tiled_a1(c.st, tn, N2, max_nu, a.dp, dv, dl, a.du, a.dul, a.df, a.ddv, c1, c2, a.ddi, a.ddo, a.dx, a.dr));
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
// FP32 records (bits of the floats, as stored).  f3: rec[4e..4e+2] = v[3e..3e+2], rec[4e+3] = loc[e].  sb_f32: per 3x3 block
// ten words a0 .. a8, column.
int shim_pack_f3(int64_t n, const float* v, const uint16_t* loc, uint32_t* rec) {
  Call c;
  const float* dv = c.in(v, (size_t)(3 * n));
  const uint16_t* dl = c.in(loc, (size_t)n);
  uint32_t* drec = c.io(rec, (size_t)(4 * n));
  SHIM_RUN(c, "launch_pack_f3", launch_pack_f3(c.st, n, dv, dl, drec));
}
int shim_pack_sb_f32(int64_t nb, const float* v, const int32_t* col, uint32_t* rec) {
  Call c;
  const float* dv = c.in(v, (size_t)(9 * nb));
  const int32_t* dc = c.in(col, (size_t)nb);
  uint32_t* drec = c.io(rec, (size_t)(10 * nb));
  SHIM_RUN(c, "launch_pack_sb_f32", launch_pack_sb_f32(c.st, nb, dv, dc, drec));
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
// rec: the records of launch_pack_sb_f32 (10 words per block)
int shim_sweep_sb_r(int64_t nS, const int64_t* sb_ptr, const uint32_t* rec, const float* binv12, float c1, float c2, float* din,
                    float* dout, float* x, float* r) {
  Call c;
  const int64_t nb = sb_ptr[nS];
  const int64_t* dp = c.in(sb_ptr, (size_t)nS + 1);
  const uint32_t* drec = c.in(rec, (size_t)(10 * nb));
  const float* dbi = c.in(binv12, (size_t)(12 * nS));
  float* ddi = c.io(din, (size_t)(4 * nS));
  float* ddo = c.io(dout, (size_t)(4 * nS));
  float* dx = c.io(x, (size_t)(4 * nS));
  float* dr = c.io(r, (size_t)(4 * nS));
  SHIM_RUN(c, "launch_sweep_sb_r", launch_sweep_sb_r(c.st, nS, dp, drec, dbi, c1, c2, ddi, ddo, dx, dr));
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
// FP64 values in CSR order with the 16-bit tile-local columns ploc; tiles of tile_rows rows: tile_uptr, ulist
int shim_sweep_schur_tiled_f64(int tile_rows, int64_t n, int max_nu, const int64_t* rowptr, const double* vals, const uint16_t* ploc,
                               const int64_t* tile_uptr, const int32_t* ulist, const int64_t* diagpos, double c1, double c2,
                               double* din, double* dout, double* x, double* r) {
  Call c;
  const int64_t nnz = rowptr[n], nt = (n + tile_rows - 1) / tile_rows;
  const int64_t* dp = c.in(rowptr, (size_t)n + 1);
  const double* dv = c.in(vals, (size_t)nnz);
  const uint16_t* dl = c.in(ploc, (size_t)nnz);
  const int64_t* du = c.in(tile_uptr, (size_t)nt + 1);
  const int32_t* dul = c.in(ulist, (size_t)tile_uptr[nt]);
  const int64_t* dg = c.in(diagpos, (size_t)n);
  double* ddi = c.io(din, (size_t)n);
  double* ddo = c.io(dout, (size_t)n);
  double* dx = c.io(x, (size_t)n);
  double* dr = c.io(r, (size_t)n);
  SHIM_RUN(c, "launch_sweep_schur_tiled_f64",
           launch_sweep_schur_tiled_f64(c.st, tile_rows, n, max_nu, dp, dv, dl, du, dul, dg, c1, c2, ddi, ddo, dx, dr));
}

int shim_tile_limit() { return tile_limit(); }

// The preconditioner's Chebyshev schedule (fsi_cheb.hpp), host only: init() and 2 n coefficient pairs - n from a new
// generator, then n more after restart()
int shim_cheb_coefficients(double lmax, double kappa, int fourth, int n, double* c1, double* c2, double* init) {
  ChebSchedule gen(lmax, kappa, fourth != 0);
  *init = gen.init();
  for (int k = 0; k < 2 * n; ++k) {
    if (k == n) gen.restart();
    gen.next(&c1[k], &c2[k]);
  }
  return 0;
}

// ---- fsi_gcr_host.hpp: the host side of the recycled GCR, no device call ------------------------------------------------------
// One operation on a store the shim keeps, then the store's whole state: born [cap], free [cap] (the first scal[3] entries),
// hot [GCR_WINDOW], scal = {hw, made, hot_next, free.size()}.  op 0 init(arg), 1 full() -> res[0], 2 take() -> res[0] slot,
// res[1] clear, 3 retire(arg) -> res[0] count, res[1..] slots, 4 window_put(arg) -> res[0] column, 5 window_drop_retired() ->
// res[0] count, res[1..] columns, 6 set_born(arg), 7 window_cols() -> res[0], 8 reset(), 9 clear_window(), 10 lead() -> res[0],
// 11 abandon(arg) -> res[0] the column to zero or -1.  res: [cap + 1] at least.
int shim_gcr_store_op(int op, int64_t arg, int32_t* res, int64_t* born, int32_t* free_slots, int32_t* hot, int64_t* scal) {
  static GcrStore s;
  if (op != 0 && s.cap == 0) { g_err = "shim_gcr_store_op: no store (op 0 first)"; return 1; }
  switch (op) {
    case 0: s = GcrStore(); s.init(arg); break;
    case 1: res[0] = s.full(); break;
    case 2: { bool clear = false; res[0] = s.take(&clear); res[1] = clear; break; }
    case 3: { const std::vector<int32_t> out = s.retire((int)arg); res[0] = (int32_t)out.size(); std::copy(out.begin(), out.end(), res + 1); break; }
    case 4: res[0] = s.window_put((int)arg); break;
    case 5: { const std::vector<int> out = s.window_drop_retired(); res[0] = (int32_t)out.size(); std::copy(out.begin(), out.end(), res + 1); break; }
    case 6: s.set_born((int)arg); break;
    case 7: res[0] = s.window_cols(); break;
    case 8: s.reset(); break;
    case 9: s.clear_window(); break;
    case 10: res[0] = (int32_t)s.lead(); break;
    case 11: res[0] = s.abandon((int)arg); break;
    default: g_err = "shim_gcr_store_op: unknown operation"; return 1;
  }
  std::copy(s.born.begin(), s.born.end(), born);
  std::copy(s.free.begin(), s.free.end(), free_slots);
  std::copy(s.hot_slots.begin(), s.hot_slots.end(), hot);
  scal[0] = s.hw; scal[1] = s.made; scal[2] = s.hot_next; scal[3] = (int64_t)s.free.size();
  return 0;
}
// out = {GCR_WINDOW, GCR_FLUSH_BATCH, gcr_ring(cap), gcr_retire_batch(cap), gcr_coef_len(cap), and of GcrStaging{cap}: sums(m),
// lagged(m), updated(m), window(), size()}
int shim_gcr_sizes(int64_t cap, int m, int64_t* out) {
  const GcrStaging lay{cap};
  const int64_t v[10] = {GCR_WINDOW, GCR_FLUSH_BATCH, gcr_ring(cap), gcr_retire_batch(cap), (int64_t)gcr_coef_len(cap),
                         lay.sums(m), lay.lagged(m), lay.updated(m), lay.window(), (int64_t)lay.size()};
  std::copy(v, v + 10, out);
  return 0;
}
// the text of a room-rule refusal (fsi_room.hpp) into out[cap], zero-terminated; host only
int shim_room_refusal(const char* fn, const char* subject, double need, const char* layout, int64_t free_b, double reserve, char* out,
                      int64_t cap) {
  const std::string text = host::room_refusal(fn, subject, need, layout, (size_t)free_b, reserve);
  if ((int64_t)text.size() >= cap) { g_err = "shim_room_refusal: the text does not fit"; return 1; }
  std::copy(text.c_str(), text.c_str() + text.size() + 1, out);
  return 0;
}
// GcrCycle: knew directions added in turn - slots [knew], over ms[k] columns with coefficients htot [knew][cap], wn, alpha
// [knew] - give y [cap] and cn [knew][cap]; pack [(gcr_flush_width(knew) + 1) m]: what a flush over m columns uploads; then
// clear(), after which nothing may be pending
int shim_gcr_cycle_algebra(int64_t cap, int knew, const int32_t* slots, const int32_t* ms, const double* htot, const double* wn,
                           const double* alpha, double* y, double* cn, int m, double* pack) {
  GcrCycle cy(cap);
  for (int k = 0; k < knew; ++k) cy.add(slots[k], htot + (size_t)k * cap, ms[k], wn[k], alpha[k]);
  if (cy.knew() != knew || !cy.pending(m)) { g_err = "shim_gcr_cycle_algebra: nothing pending after add()"; return 1; }
  std::copy(cy.y.begin(), cy.y.end(), y);
  for (int k = 0; k < knew; ++k) std::copy(cy.cn[k].begin(), cy.cn[k].end(), cn + (size_t)k * cap);
  const std::vector<double> p = cy.pack(m, gcr_flush_width(knew));
  std::copy(p.begin(), p.end(), pack);
  cy.clear();
  if (cy.knew() != 0 || cy.pending((int)cap)) { g_err = "shim_gcr_cycle_algebra: pending after clear()"; return 1; }
  return 0;
}
// the policies: the status is the answer (gcr_cycle_end: 0 go, 1 stagnated, 2 stalled; the predicates: 0 / 1)
int shim_gcr_cycle_end(int since_gain, int f32, double rnorm, double target, double r_entry, int store_full) {
  return (int)gcr_cycle_end(since_gain, f32 != 0, rnorm, target, r_entry, store_full != 0);
}
int shim_gcr_orth_lost(const double* h, int m, double w2, double wn2, double floor) { return gcr_orth_lost(h, m, w2, wn2, floor); }
int shim_gcr_verdict_due(double rtol, double rnorm, double bnorm, int cyc, int cycle_its, int stagnated, int stalled, int store_full,
                         int fell_back, int suspect) {
  return gcr_verdict_due(GcrVerdictIn{rtol, rnorm, bnorm, cyc, cycle_its, stagnated != 0, stalled != 0, store_full != 0}, fell_back != 0, suspect != 0);
}
int shim_gcr_verdict_skippable(double rtol, double rnorm, double bnorm, int cyc, int cycle_its, int stagnated, int stalled,
                               int store_full, int in_newton, int final_cycle, double skip_rtol, double last_drift) {
  return gcr_verdict_skippable(GcrVerdictIn{rtol, rnorm, bnorm, cyc, cycle_its, stagnated != 0, stalled != 0, store_full != 0},
                               in_newton != 0, final_cycle != 0, skip_rtol, last_drift);
}
// out = {gcr_reorth_threshold(f32, part, rtol_floor, forced), gcr_adaptive_start(rtol, utol, utol_ratio, utol_floor),
// gcr_adaptive_tighten(rtol, utol, b_unscaled, ru, utol_floor), gcr_basis_fp32(tol_hint, rtol, fp32_floor)} from in = {f32, part,
// rtol_floor, forced, rtol, utol, utol_ratio, utol_floor, b_unscaled, ru, tol_hint, fp32_floor}
int shim_gcr_tolerances(const double* in, double* out) {
  out[0] = gcr_reorth_threshold(in[0] != 0.0, in[1] != 0.0, in[2], in[3]);
  out[1] = gcr_adaptive_start(in[4], in[5], in[6], in[7]);
  out[2] = gcr_adaptive_tighten(in[4], in[5], in[8], in[9], in[7]);
  out[3] = gcr_basis_fp32(in[10], in[4], in[11]) ? 1.0 : 0.0;
  return 0;
}

// ---- fsi_solver.hip / fsi_product.hip: the monolithic matrix's structure and products -----------------------------------------
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
// launch_product on the FP64 matrix, all six value rows (ad64 null) or the d rows in pair form; vrank, nadj_ptr, nadj may each
// be null (npairs: the length of nadj, and ad64 holds 6 npairs)
int shim_spmv_node6(int64_t N2, int64_t V, const int64_t* rowptr, const int32_t* cols, const double* vals, const int32_t* vrank,
                    const int64_t* nadj_ptr, const int32_t* nadj, int64_t npairs, const double* x, double* y, const double* ad64) {
  Call c;
  const int64_t n = 6 * N2 + V;
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n]);
  const double* dv = c.in(vals, (size_t)rowptr[n]);
  ProductView m;
  m.N2 = N2; m.V = V; m.rowptr = drp; m.cols = dc; m.vals = dv;
  m.g = PRowGraph{c.in(vrank, (size_t)V), c.in(nadj_ptr, (size_t)N2 + 1), c.in(nadj, (size_t)npairs)};
  const double* dx = c.in(x, (size_t)n);
  double* dy = c.io(y, (size_t)n);
  m.ad64 = c.in(ad64, (size_t)(6 * npairs));
  SHIM_RUN_STATUS(c, "launch_product (six rows / pair form)", launch_product(c.st, m, m.ad64 ? PRODUCT_PAIR64 : PRODUCT_SIX64, dx, dy));
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
// the split pair form as a refresh builds it: launch_drows_extract_split, launch_drows_offsets and, when doff[N2] <= dvcap pairs,
// launch_drows_gather_dv.  Node rows only as above; dd [3 npairs], cdeg [N2], doff [N2 + 1], dv [3 dvcap]
int shim_drows_split(int64_t N2, const int64_t* rowptr, const double* A, const int64_t* nadj_ptr, double* ad64, int32_t* flag,
                     double* dd, int32_t* cdeg, int64_t* doff, double* dv, int64_t dvcap) {
  Call c;
  const int64_t npairs = nadj_ptr[N2];
  const int64_t* drp = c.in(rowptr, (size_t)(6 * N2) + 1);
  const double* dA = c.in(A, (size_t)rowptr[6 * N2]);
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  double* d64 = c.io(ad64, (size_t)(6 * npairs));
  int32_t* df = c.io(flag, 1);
  double* ddd = c.io(dd, (size_t)(3 * npairs));
  int32_t* dcd = c.io(cdeg, (size_t)N2);
  int64_t* dof = c.io(doff, (size_t)N2 + 1);
  double* ddv = c.io(dv, (size_t)(3 * dvcap));
  if (c.ok()) {
    launch_drows_extract_split(c.st, N2, drp, dA, dnp, d64, nullptr, df, ddd, dcd);
    launch_drows_offsets(c.st, N2, dcd, dof);
    int64_t total = -1;
    c.note(hipMemcpyAsync(&total, dof + N2, sizeof total, hipMemcpyDeviceToHost, c.st));
    c.note(hipStreamSynchronize(c.st));
    if (c.ok() && total > 0 && total <= dvcap) launch_drows_gather_dv(c.st, N2, dnp, dof, d64, ddv);
  }
  return c.finish("launch_drows_extract_split / launch_drows_offsets / launch_drows_gather_dv");
}
// launch_product in the split form: dd [3 npairs], dv [3 ndv] (may be null), doff [N2 + 1]; the rest as shim_spmv_node6
int shim_spmv_node6s(int64_t N2, int64_t V, const int64_t* rowptr, const int32_t* cols, const double* vals, const int32_t* vrank,
                     const int64_t* nadj_ptr, const int32_t* nadj, int64_t npairs, const double* x, double* y, const double* dd,
                     const double* dv, int64_t ndv, const int64_t* doff) {
  Call c;
  const int64_t n = 6 * N2 + V;
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n]);
  const double* dvl = c.in(vals, (size_t)rowptr[n]);
  ProductView m;
  m.N2 = N2; m.V = V; m.rowptr = drp; m.cols = dc; m.vals = dvl;
  m.g = PRowGraph{c.in(vrank, (size_t)V), c.in(nadj_ptr, (size_t)N2 + 1), c.in(nadj, (size_t)npairs)};
  const double* dx = c.in(x, (size_t)n);
  double* dy = c.io(y, (size_t)n);
  m.dd = c.in(dd, (size_t)(3 * npairs));
  m.dv = c.in(dv, (size_t)(3 * ndv));
  m.doff = c.in(doff, (size_t)N2 + 1);
  SHIM_RUN_STATUS(c, "launch_product (split form)", launch_product(c.st, m, PRODUCT_SPLIT64, dx, dy));
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
// launch_product on the padded FP32 copy, six rows (ad32 null) or pair form.  vals [n32]; the pressure rows' values at vals + tail_shift + rowptr[row]; ad32 [6 npairs] or null
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
  ProductView m;
  m.N2 = N2; m.V = V; m.rowptr = drp; m.cols = dc; m.p32 = dp; m.cols32 = dc32; m.vals32 = dv; m.tail_shift = tail_shift;
  m.g = PRowGraph{c.in(vrank, (size_t)V), c.in(nadj_ptr, (size_t)N2 + 1), c.in(nadj, (size_t)npairs)};
  const double* dx = c.in(x, (size_t)n);
  double* dy = c.io(y, (size_t)n);
  m.ad32 = c.in(ad32, (size_t)(6 * npairs));
  SHIM_RUN_STATUS(c, "launch_product (padded FP32 copy)", launch_product(c.st, m, m.ad32 ? PRODUCT_PAIR32 : PRODUCT_SIX32, dx, dy));
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

// ---- the two-level (P2 -> P1) coarse levels and the diagonal scalings (fsi_block.hip) ---------------------------------------
// Every flags / rowmax_bits argument is in/out (four / one int32), so that a test can pre-fill it.  Vectors of nodes are float4.
// db [3 nnz], rowscale [6 N2], rowflag [3 N2] with nnz = nadj_ptr[N2]; d0 [N2]; flags [4]
int shim_mg_d0(int64_t N2, const int64_t* nadj_ptr, const int32_t* nadj, const double* db, const double* rowscale,
               const uint8_t* rowflag, float* d0, int32_t* flags) {
  Call c;
  const int64_t nnz = nadj_ptr[N2];
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)nnz);
  const double* ddb = c.in(db, 3 * (size_t)nnz);
  const double* drs = c.in(rowscale, 6 * (size_t)N2);
  const uint8_t* drf = c.in(rowflag, 3 * (size_t)N2);
  float* dd0 = c.io(d0, (size_t)N2);
  int32_t* dfl = c.io(flags, 4);
  SHIM_RUN(c, "launch_mg_d0", launch_mg_d0(c.st, N2, dnp, dn, ddb, drs, drf, dd0, dfl));
}
// chptr [nc+1], child / chw [chptr[nc]], par / pw [2 N2], cptr [nc+1], ccol / Ac [cptr[nc]]
int shim_mg_rap(int64_t nc, int64_t N2, const int64_t* chptr, const int32_t* child, const float* chw, const int64_t* nadj_ptr,
                const int32_t* nadj, const double* db, const double* rowscale, const uint8_t* rowflag, const int32_t* par,
                const float* pw, const int64_t* cptr, const int32_t* ccol, double* Ac, int32_t* flags) {
  Call c;
  const int64_t nnz = nadj_ptr[N2], nch = chptr[nc], cnnz = cptr[nc];
  const int64_t* dchp = c.in(chptr, (size_t)nc + 1);
  const int32_t* dch = c.in(child, (size_t)nch);
  const float* dchw = c.in(chw, (size_t)nch);
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)nnz);
  const double* ddb = c.in(db, 3 * (size_t)nnz);
  const double* drs = c.in(rowscale, 6 * (size_t)N2);
  const uint8_t* drf = c.in(rowflag, 3 * (size_t)N2);
  const int32_t* dpar = c.in(par, 2 * (size_t)N2);
  const float* dpw = c.in(pw, 2 * (size_t)N2);
  const int64_t* dcp = c.in(cptr, (size_t)nc + 1);
  const int32_t* dcc = c.in(ccol, (size_t)cnnz);
  double* dAc = c.io(Ac, (size_t)cnnz);
  int32_t* dfl = c.io(flags, 4);
  SHIM_RUN(c, "launch_mg_rap", launch_mg_rap(c.st, nc, dchp, dch, dchw, dnp, dn, ddb, drs, drf, dpar, dpw, dcp, dcc, dAc, dfl));
}
// cfine [nc], rowflag [3 N2]; cc [cptr[nc]], cflag [3 nc], dcinv4 [4 nc], rowmax_bits [1]
int shim_mg_coarse_finish(int64_t nc, int64_t N2, const int64_t* cptr, const int32_t* ccol, const double* Ac, const int32_t* cfine,
                          const uint8_t* rowflag, float* cc, uint8_t* cflag, float* dcinv4, int32_t* rowmax_bits) {
  Call c;
  const int64_t cnnz = cptr[nc];
  const int64_t* dcp = c.in(cptr, (size_t)nc + 1);
  const int32_t* dcc = c.in(ccol, (size_t)cnnz);
  const double* dAc = c.in(Ac, (size_t)cnnz);
  const int32_t* dcf = c.in(cfine, (size_t)nc);
  const uint8_t* drf = c.in(rowflag, 3 * (size_t)N2);
  float* dcv = c.io(cc, (size_t)cnnz);
  uint8_t* dcfl = c.io(cflag, 3 * (size_t)nc);
  float* ddi = c.io(dcinv4, 4 * (size_t)nc);
  int32_t* drm = c.io(rowmax_bits, 1);
  SHIM_RUN(c, "launch_mg_coarse_finish", launch_mg_coarse_finish(c.st, nc, dcp, dcc, dAc, dcf, drf, dcv, dcfl, ddi, drm));
}
// d0 / r4: [N2] / [4 N2]; dcinv4, rc4 and the optional Chebyshev start cx / cr / cd (all null or none): [4 nc]
int shim_mg_restrict(int64_t nc, int64_t N2, const int64_t* chptr, const int32_t* child, const float* chw, const float* d0,
                     const float* r4, const float* dcinv4, float* rc4, float inv_theta, float* cx, float* cr, float* cd) {
  Call c;
  const int64_t nch = chptr[nc];
  const int64_t* dchp = c.in(chptr, (size_t)nc + 1);
  const int32_t* dch = c.in(child, (size_t)nch);
  const float* dchw = c.in(chw, (size_t)nch);
  const float* dd0 = c.in(d0, (size_t)N2);
  const float* dr4 = c.in(r4, 4 * (size_t)N2);
  const float* ddi = c.in(dcinv4, 4 * (size_t)nc);
  float* drc = c.io(rc4, 4 * (size_t)nc);
  float* dcx = c.io(cx, 4 * (size_t)nc);
  float* dcr = c.io(cr, 4 * (size_t)nc);
  float* dcd = c.io(cd, 4 * (size_t)nc);
  SHIM_RUN(c, "launch_mg_restrict", launch_mg_restrict(c.st, nc, dchp, dch, dchw, dd0, dr4, ddi, drc, inv_theta, dcx, dcr, dcd));
}
// par / pw [2 N2], d0 [N2], xc4 [4 nc], e4 [4 N2]
int shim_mg_prolong(int64_t N2, int64_t nc, const int32_t* par, const float* pw, const float* d0, const float* xc4, float* e4) {
  Call c;
  const int32_t* dpar = c.in(par, 2 * (size_t)N2);
  const float* dpw = c.in(pw, 2 * (size_t)N2);
  const float* dd0 = c.in(d0, (size_t)N2);
  const float* dxc = c.in(xc4, 4 * (size_t)nc);
  float* de = c.io(e4, 4 * (size_t)N2);
  SHIM_RUN(c, "launch_mg_prolong", launch_mg_prolong(c.st, N2, dpar, dpw, dd0, dxc, de));
}
// sb_ptr [nS+1], sb_col [sb_ptr[nS]], vals [9 sb_ptr[nS]], flag [nS]
int shim_sbmg_flags(int64_t nS, const int64_t* sb_ptr, const int32_t* sb_col, const float* vals, uint8_t* flag) {
  Call c;
  const int64_t nb = sb_ptr[nS];
  const int64_t* dsp = c.in(sb_ptr, (size_t)nS + 1);
  const int32_t* dsc = c.in(sb_col, (size_t)nb);
  const float* dv = c.in(vals, 9 * (size_t)nb);
  uint8_t* dfl = c.io(flag, (size_t)nS);
  SHIM_RUN(c, "launch_sbmg_flags", launch_sbmg_flags(c.st, nS, dsp, dsc, dv, dfl));
}
// snode / flag [nS], rowscale [6 N2], par / pw [2 nS]; cvals [9 cptr[nc]]
int shim_sbmg_rap(int64_t nc, int64_t nS, int64_t N2, const int64_t* chptr, const int32_t* child, const float* chw,
                  const int64_t* sb_ptr, const int32_t* sb_col, const float* vals, const int32_t* snode, const double* rowscale,
                  const uint8_t* flag, const int32_t* par, const float* pw, const int64_t* cptr, const int32_t* ccol, float* cvals,
                  int32_t* flags) {
  Call c;
  const int64_t nb = sb_ptr[nS], nch = chptr[nc], cnnz = cptr[nc];
  const int64_t* dchp = c.in(chptr, (size_t)nc + 1);
  const int32_t* dch = c.in(child, (size_t)nch);
  const float* dchw = c.in(chw, (size_t)nch);
  const int64_t* dsp = c.in(sb_ptr, (size_t)nS + 1);
  const int32_t* dsc = c.in(sb_col, (size_t)nb);
  const float* dv = c.in(vals, 9 * (size_t)nb);
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const double* drs = c.in(rowscale, 6 * (size_t)N2);
  const uint8_t* dfl = c.in(flag, (size_t)nS);
  const int32_t* dpar = c.in(par, 2 * (size_t)nS);
  const float* dpw = c.in(pw, 2 * (size_t)nS);
  const int64_t* dcp = c.in(cptr, (size_t)nc + 1);
  const int32_t* dcc = c.in(ccol, (size_t)cnnz);
  float* dcv = c.io(cvals, 9 * (size_t)cnnz);
  int32_t* dflags = c.io(flags, 4);
  SHIM_RUN(c, "launch_sbmg_rap",
           launch_sbmg_rap(c.st, nc, dchp, dch, dchw, dsp, dsc, dv, dsn, drs, dfl, dpar, dpw, dcp, dcc, dcv, dflags));
}
// cvals [9 cptr[nc]] in place, cfine [nc], flag [nS]; cbinv12 [12 nc], cflag [nc], rowmax_bits [1]
int shim_sbmg_coarse_finish(int64_t nc, int64_t nS, const int64_t* cptr, const int32_t* ccol, float* cvals, const int32_t* cfine,
                            const uint8_t* flag, float* cbinv12, uint8_t* cflag, int32_t* rowmax_bits) {
  Call c;
  const int64_t cnnz = cptr[nc];
  const int64_t* dcp = c.in(cptr, (size_t)nc + 1);
  const int32_t* dcc = c.in(ccol, (size_t)cnnz);
  float* dcv = c.io(cvals, 9 * (size_t)cnnz);
  const int32_t* dcf = c.in(cfine, (size_t)nc);
  const uint8_t* dfl = c.in(flag, (size_t)nS);
  float* dbi = c.io(cbinv12, 12 * (size_t)nc);
  uint8_t* dcfl = c.io(cflag, (size_t)nc);
  int32_t* drm = c.io(rowmax_bits, 1);
  SHIM_RUN(c, "launch_sbmg_coarse_finish", launch_sbmg_coarse_finish(c.st, nc, dcp, dcc, dcv, dcf, dfl, dbi, dcfl, drm));
}
// r4 [4 nS], rc4 [4 nc]; the optional exact-solve right-hand side: bpos [nc], bd [nbd] (both null or neither)
int shim_sbmg_restrict(int64_t nc, int64_t nS, int64_t N2, const int64_t* chptr, const int32_t* child, const float* chw,
                       const int32_t* snode, const double* rowscale, const uint8_t* flag, const uint8_t* cflag, const float* r4,
                       float* rc4, const int32_t* bpos, double* bd, int64_t nbd) {
  Call c;
  const int64_t nch = chptr[nc];
  const int64_t* dchp = c.in(chptr, (size_t)nc + 1);
  const int32_t* dch = c.in(child, (size_t)nch);
  const float* dchw = c.in(chw, (size_t)nch);
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const double* drs = c.in(rowscale, 6 * (size_t)N2);
  const uint8_t* dfl = c.in(flag, (size_t)nS);
  const uint8_t* dcfl = c.in(cflag, (size_t)nc);
  const float* dr4 = c.in(r4, 4 * (size_t)nS);
  float* drc = c.io(rc4, 4 * (size_t)nc);
  const int32_t* dbp = c.in(bpos, (size_t)nc);
  double* dbd = c.io(bd, (size_t)nbd);
  SHIM_RUN(c, "launch_sbmg_restrict", launch_sbmg_restrict(c.st, nc, dchp, dch, dchw, dsn, drs, dfl, dcfl, dr4, drc, dbp, dbd));
}
// par / pw [2 nS], flag [nS], xc4 [4 nc] (may be null with xd), e4 [4 nS]; the optional exact-solve answer: bpos [nc], xd [nxd]
int shim_sbmg_prolong(int64_t nS, int64_t nc, const int32_t* par, const float* pw, const uint8_t* flag, const float* xc4, float* e4,
                      const int32_t* bpos, const double* xd, int64_t nxd) {
  Call c;
  const int32_t* dpar = c.in(par, 2 * (size_t)nS);
  const float* dpw = c.in(pw, 2 * (size_t)nS);
  const uint8_t* dfl = c.in(flag, (size_t)nS);
  const float* dxc = c.in(xc4, 4 * (size_t)nc);
  float* de = c.io(e4, 4 * (size_t)nS);
  const int32_t* dbp = c.in(bpos, (size_t)nc);
  const double* dxd = c.in(xd, (size_t)nxd);
  SHIM_RUN(c, "launch_sbmg_prolong", launch_sbmg_prolong(c.st, nS, dpar, dpw, dfl, dxc, de, dbp, dxd));
}
// snode [nS], diagpos3 [3 N2], Avv [nA]; binv12 [12 nS], binv9 [9 nS]
int shim_sb_binv(int64_t nS, int64_t N2, const int32_t* snode, const int64_t* diagpos3, const double* Avv, int64_t nA, float* binv12,
                 double* binv9) {
  Call c;
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const int64_t* ddp = c.in(diagpos3, 3 * (size_t)N2);
  const double* dA = c.in(Avv, (size_t)nA);
  float* db12 = c.io(binv12, 12 * (size_t)nS);
  double* db9 = c.io(binv9, 9 * (size_t)nS);
  SHIM_RUN(c, "launch_sb_binv", launch_sb_binv(c.st, nS, dsn, ddp, dA, db12, db9));
}
// dinv [4 nS]
int shim_sb_dinv(int64_t nS, int64_t N2, const int32_t* snode, const int64_t* diagpos3, const double* Avv, int64_t nA, float* dinv) {
  Call c;
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const int64_t* ddp = c.in(diagpos3, 3 * (size_t)N2);
  const double* dA = c.in(Avv, (size_t)nA);
  float* ddi = c.io(dinv, 4 * (size_t)nS);
  SHIM_RUN(c, "launch_sb_dinv", launch_sb_dinv(c.st, nS, dsn, ddp, dA, ddi));
}
// mask (may be null) / diagpos [3 nn], A [nA], dinv4 [4 nn]
int shim_dinv_f32(int64_t nn, const double* mask, const int64_t* diagpos, const double* A, int64_t nA, float* dinv4) {
  Call c;
  const double* dm = c.in(mask, 3 * (size_t)nn);
  const int64_t* ddp = c.in(diagpos, 3 * (size_t)nn);
  const double* dA = c.in(A, (size_t)nA);
  float* ddi = c.io(dinv4, 4 * (size_t)nn);
  SHIM_RUN(c, "launch_dinv_f32", launch_dinv_f32(c.st, nn, dm, ddp, dA, ddi));
}
// diagpos / dinv [n], A [nA]
int shim_diag_inverse(int64_t n, const int64_t* diagpos, const double* A, int64_t nA, double* dinv) {
  Call c;
  const int64_t* ddp = c.in(diagpos, (size_t)n);
  const double* dA = c.in(A, (size_t)nA);
  double* ddi = c.io(dinv, (size_t)n);
  SHIM_RUN(c, "launch_diag_inverse", launch_diag_inverse(c.st, n, ddp, dA, ddi));
}
// binv9 [9 nS], y [3 nS] in place
int shim_block_scale_d(int64_t nS, const double* binv9, double* y) {
  Call c;
  const double* db9 = c.in(binv9, 9 * (size_t)nS);
  double* dy = c.io(y, 3 * (size_t)nS);
  SHIM_RUN(c, "launch_block_scale_d", launch_block_scale_d(c.st, nS, db9, dy));
}
// snode [nS], full [nfull], binv12 [12 nS]; x, r, d, d2 [4 nS]
int shim_solid_cycle_init(int64_t nS, int64_t nfull, const int32_t* snode, const double* full, const float* binv12, float scale,
                          float* x, float* r, float* d, float* d2) {
  Call c;
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const double* dfu = c.in(full, (size_t)nfull);
  const float* db12 = c.in(binv12, 12 * (size_t)nS);
  float* dx = c.io(x, 4 * (size_t)nS);
  float* dr = c.io(r, 4 * (size_t)nS);
  float* dd = c.io(d, 4 * (size_t)nS);
  float* dd2 = c.io(d2, 4 * (size_t)nS);
  SHIM_RUN(c, "launch_solid_cycle_init", launch_solid_cycle_init(c.st, nS, dsn, dfu, db12, scale, dx, dr, dd, dd2));
}
// comp [4 nS]
int shim_gather3_f32(int64_t nS, int64_t nfull, const int32_t* snode, const double* full, float* comp) {
  Call c;
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const double* dfu = c.in(full, (size_t)nfull);
  float* dco = c.io(comp, 4 * (size_t)nS);
  SHIM_RUN(c, "launch_gather3_f32", launch_gather3_f32(c.st, nS, dsn, dfu, dco));
}
// full [nfull] in place
int shim_scatter3_f32(int64_t nS, int64_t nfull, const int32_t* snode, const float* comp, double* full) {
  Call c;
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const float* dco = c.in(comp, 4 * (size_t)nS);
  double* dfu = c.io(full, (size_t)nfull);
  SHIM_RUN(c, "launch_scatter3_f32", launch_scatter3_f32(c.st, nS, dsn, dco, dfu));
}

// ---- fsi_bcr.hip: the exact coarse solve by block cyclic reduction -----------------------------------------------------------
// Descriptors come as flat int64 / double rows (no dependence on the structs' padding); the tile lists are built by the
// planner's own builders (fsi_bcr.hpp).  Every descriptor is checked against the array lengths first: status LAUNCH_REFUSED
// (nothing launched) for one that would reach outside them.
namespace {
bool within(int64_t first, int64_t last, int64_t n) { return first >= 0 && last >= first && last < n; }
int refuse(const char* what, int64_t i) {
  g_err = std::string(what) + ": descriptor " + std::to_string(i) + " reaches outside its arrays, nothing launched";
  return LAUNCH_REFUSED;
}
}  // namespace

// desc [ninv][6]: a, o32 (-1: no FP32 copy), cb, rb, m, ld32 - in place on arena64 [n64], copies into arena32 [n32]; flag [1]
int shim_bcr_invert(int64_t ninv, const int64_t* desc, double* arena64, int64_t n64, float* arena32, int64_t n32, int32_t* flag) {
  std::vector<BcrInv> invs;
  std::vector<BcrGemm> gemms;
  std::vector<BcrGemmTile> tiles;
  int maxm = 0;
  for (int64_t i = 0; i < ninv; ++i) {
    const int64_t* q = desc + 6 * i;
    const int m = (int)q[4];
    const BcrInv v = bcr_inverse(q[0], q[1], q[2], q[3], m, (int)q[5]);
    if (m < 1 || !within(v.a, v.a + (int64_t)m * m - 1, n64) || !within(v.cb, v.cb + (int64_t)m * BCR_PANEL - 1, n64) ||
        !within(v.rb, v.rb + (int64_t)m * BCR_PANEL - 1, n64) || (v.o32 >= 0 && (v.ld32 < m || !within(v.o32, v.o32 + (int64_t)(m - 1) * v.ld32 + m - 1, n32))))
      return refuse("shim_bcr_invert", i);
    invs.push_back(v);
    bcr_gemm_tiles(bcr_inverse_update(v), (int32_t)gemms.size(), tiles);
    gemms.push_back(bcr_inverse_update(v));
    maxm = std::max(maxm, m);
  }
  Call c;
  const BcrInv* dinv = c.in(invs.data(), invs.size());
  const BcrGemm* dg = c.in(gemms.data(), gemms.size());
  const BcrGemmTile* dt = c.in(tiles.data(), tiles.size());
  double* d64 = c.io(arena64, (size_t)n64);
  float* d32 = c.io(arena32, (size_t)n32);
  int32_t* df = c.io(flag, 1);
  SHIM_RUN(c, "launch_bcr_invert", launch_bcr_invert(c.st, dinv, ninv, dt, (int64_t)tiles.size(), dg, maxm, d64, d32, df));
}
// idesc [ng][16]: a1, b1, a2, b2, c, o32, M, N, K1, K2, lda1, ldb1, lda2, ldb2, ldc, ld32; ddesc [ng][2]: alpha, beta; flag [1]
int shim_bcr_gemm(int64_t ng, const int64_t* idesc, const double* ddesc, double* arena64, int64_t n64, float* arena32, int64_t n32,
                  int32_t* flag) {
  std::vector<BcrGemm> gemms;
  std::vector<BcrGemmTile> tiles;
  for (int64_t i = 0; i < ng; ++i) {
    const int64_t* q = idesc + 16 * i;
    BcrGemm g{q[0], q[1], q[2], q[3], q[4], q[5], (int32_t)q[6], (int32_t)q[7], (int32_t)q[8], (int32_t)q[9], (int32_t)q[10],
              (int32_t)q[11], (int32_t)q[12], (int32_t)q[13], (int32_t)q[14], (int32_t)q[15], ddesc[2 * i], ddesc[2 * i + 1]};
    bool ok = g.M >= 1 && g.N >= 1;
    for (int prod = 0; prod < 2 && ok; ++prod) {
      const int64_t ao = prod ? g.a2 : g.a1, bo = prod ? g.b2 : g.b1;
      const int64_t K = prod ? g.K2 : g.K1, lda = prod ? g.lda2 : g.lda1, ldb = prod ? g.ldb2 : g.ldb1;
      if (ao < 0 || bo < 0 || K <= 0) continue;
      ok = lda >= K && ldb >= g.N && within(ao, ao + (g.M - 1) * lda + K - 1, n64) && within(bo, bo + (K - 1) * ldb + g.N - 1, n64);
    }
    if (ok && g.c >= 0) ok = g.ldc >= g.N && within(g.c, g.c + (int64_t)(g.M - 1) * g.ldc + g.N - 1, n64);
    if (ok && g.o32 >= 0) ok = g.ld32 >= g.N && within(g.o32, g.o32 + (int64_t)(g.M - 1) * g.ld32 + g.N - 1, n32);
    if (!ok) return refuse("shim_bcr_gemm", i);
    bcr_gemm_tiles(g, (int32_t)gemms.size(), tiles);
    gemms.push_back(g);
  }
  Call c;
  const BcrGemm* dg = c.in(gemms.data(), gemms.size());
  const BcrGemmTile* dt = c.in(tiles.data(), tiles.size());
  double* d64 = c.io(arena64, (size_t)n64);
  float* d32 = c.io(arena32, (size_t)n32);
  int32_t* df = c.io(flag, 1);
  SHIM_RUN(c, "launch_bcr_gemm", launch_bcr_gemm(c.st, dt, (int64_t)tiles.size(), dg, d64, d32, df));
}
// tdesc [nt][14]: w, rows, ldw, out, nseg, then (off, len, src) of three segments; W [nW] floats; b, x [n] (b in place when
// forward, x when backward)
int shim_bcr_apply(int forward, int64_t nt, const int64_t* tdesc, const float* W, int64_t nW, double* b, double* x, int64_t n) {
  std::vector<BcrTask> tasks;
  std::vector<BcrTile> tiles;
  int maxld = 0;
  for (int64_t i = 0; i < nt; ++i) {
    const int64_t* q = tdesc + 14 * i;
    BcrTask t{q[0], (int32_t)q[1], (int32_t)q[2], (int32_t)q[3], (int32_t)q[4], {}};
    bool ok = t.rows >= 1 && t.ldw >= 4 && t.ldw % 4 == 0 && t.w % 4 == 0 && t.ldw <= 8000 && t.nseg >= 0 && t.nseg <= 3 &&
              within(t.w, t.w + (int64_t)t.rows * t.ldw - 1, nW) && within(t.out, (int64_t)t.out + t.rows - 1, n);
    int64_t cols = 0;
    for (int k = 0; k < 3 && ok; ++k) {
      t.seg[k] = BcrSeg{(int32_t)q[5 + 3 * k], (int32_t)q[6 + 3 * k], (int32_t)q[7 + 3 * k]};
      if (k >= t.nseg) continue;
      cols += t.seg[k].len;
      ok = t.seg[k].len >= 0 && (t.seg[k].len == 0 || within(t.seg[k].off, (int64_t)t.seg[k].off + t.seg[k].len - 1, n));
    }
    if (!ok || cols > t.ldw) return refuse("shim_bcr_apply", i);
    bcr_task_tiles(t, (int32_t)tasks.size(), tiles);
    tasks.push_back(t);
    maxld = std::max(maxld, (int)t.ldw);
  }
  Call c;
  const BcrTask* dts = c.in(tasks.data(), tasks.size());
  const BcrTile* dtl = c.in(tiles.data(), tiles.size());
  const float* dW = c.in(W, (size_t)nW);
  double* db = c.io(b, (size_t)n);
  double* dx = c.io(x, (size_t)n);
  SHIM_RUN(c, "launch_bcr_apply", launch_bcr_apply(c.st, forward != 0, dtl, (int64_t)tiles.size(), dts, maxld, dW, db, dx));
}
// cvals [9 nblk], dst / ld [nblk]; arena64 [n64] in place
int shim_bcr_fill(int64_t nblk, const float* cvals, const int64_t* dst, const int32_t* ld, double shift, double* arena64, int64_t n64) {
  for (int64_t e = 0; e < nblk; ++e) {
    const int64_t l = ld[e] < 0 ? -(int64_t)ld[e] : ld[e];
    if (dst[e] >= 0 && (l < 3 || !within(dst[e], dst[e] + 2 * l + 2, n64))) return refuse("shim_bcr_fill", e);
  }
  Call c;
  const float* dcv = c.in(cvals, 9 * (size_t)nblk);
  const int64_t* dd = c.in(dst, (size_t)nblk);
  const int32_t* dl = c.in(ld, (size_t)nblk);
  double* d64 = c.io(arena64, (size_t)n64);
  SHIM_RUN(c, "launch_bcr_fill", launch_bcr_fill(c.st, nblk, dcv, dd, dl, shift, d64));
}
// pos [nc]; rc4 / xc4 [4 nc]; b / x [n]
int shim_bcr_gather(int64_t nc, const int32_t* pos, const float* rc4, double* b, int64_t n) {
  for (int64_t i = 0; i < nc; ++i) if (!within(3 * (int64_t)pos[i], 3 * (int64_t)pos[i] + 2, n)) return refuse("shim_bcr_gather", i);
  Call c;
  const int32_t* dp = c.in(pos, (size_t)nc);
  const float* dr = c.in(rc4, 4 * (size_t)nc);
  double* db = c.io(b, (size_t)n);
  SHIM_RUN(c, "launch_bcr_gather", launch_bcr_gather(c.st, nc, dp, dr, db));
}
int shim_bcr_scatter(int64_t nc, const int32_t* pos, const double* x, int64_t n, float* xc4) {
  for (int64_t i = 0; i < nc; ++i) if (!within(3 * (int64_t)pos[i], 3 * (int64_t)pos[i] + 2, n)) return refuse("shim_bcr_scatter", i);
  Call c;
  const int32_t* dp = c.in(pos, (size_t)nc);
  const double* dx = c.in(x, (size_t)n);
  float* dxc = c.io(xc4, 4 * (size_t)nc);
  SHIM_RUN(c, "launch_bcr_scatter", launch_bcr_scatter(c.st, nc, dp, dx, dxc));
}

// The whole solve on a bare context: bcr_plan on the pattern (cptr [nc + 1], ccol), then for every value set s (cvals [nsets][9
// cptr[nc]], FP32 3x3 blocks as the solid cycle's coarse level holds them) bcr_refresh with tune.bcr_shift = shift and, where it
// left the solve ready, nrhs solves two ways: rhs [nrhs][3 nc] (FP64, the solve's own order) written straight to bcr_rhs ->
// x [nsets][nrhs][3 nc]; rc4 [nrhs][4 nc] (node order) through the production gather / scatter -> xc4 [nsets][nrhs][4 nc].
// stats [12]: usable, blocks, max_block, levels, bytes32, bytes64, setup_flops, launches, planned, number of tasks, FP32 arena
// floats, FP64 arena doubles.  ready [nsets], pos [nc].  Of the last value set, when their capacities suffice: arena32 [cap32],
// tasks [cap_tasks][16] (w, rows, ldw, out, nseg, 3 x (off, len, src), level, kind 0 forward / 1 backward / 2 top), in the
// planner's order.  Any output may be null.
int shim_bcr_run(int64_t nc, const int64_t* cptr, const int32_t* ccol, int nsets, const float* cvals, double shift, int nrhs,
                 const double* rhs, const float* rc4, int64_t* stats, int32_t* ready, int32_t* pos, double* x, float* xc4,
                 float* arena32, int64_t cap32, int64_t* tasks, int64_t cap_tasks) {
  FsiCtx* ctx = new FsiCtx();
  hipError_t e = hipSuccess;
  auto note = [&](hipError_t y) { if (e == hipSuccess && y != hipSuccess) e = y; };
  note(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  ctx->tune.bcr_shift = shift;
  const int64_t nnz = cptr[nc];
  std::vector<int64_t> p(cptr, cptr + nc + 1);
  std::vector<int32_t> cc(ccol, ccol + nnz);
  host::BcrPlanStats st;
  int rc = e == hipSuccess ? host::bcr_plan(ctx, nc, p, cc, &st) : 0;
  BcrData* d = ctx->bcr;
  const bool planned = d && d->planned;
  if (stats) {
    const int64_t v[] = {st.usable, st.blocks, st.max_block, st.levels, st.bytes32, st.bytes64, st.setup_flops, st.launches, planned,
                         planned ? (int64_t)d->tasks.n : 0, planned ? (int64_t)d->arena32.n : 0, planned ? (int64_t)d->arena64.n : 0};
    std::copy(v, v + 12, stats);
  }
  const int64_t n = 3 * nc;
  float* drc = nullptr;
  float* dxc = nullptr;
  if (planned && rc == 0) {
    if (pos) note(hipMemcpy(pos, d->pos.p, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    note(ctx->sbmg_cvals.alloc(9 * (size_t)nnz));
    note(hipMalloc(&drc, 4 * (size_t)nc * sizeof(float)));
    note(hipMalloc(&dxc, 4 * (size_t)nc * sizeof(float)));
    for (int s = 0; s < nsets && e == hipSuccess && rc == 0; ++s) {
      note(hipMemcpy(ctx->sbmg_cvals.p, cvals + 9 * (size_t)nnz * s, 9 * (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
      if (e == hipSuccess) rc = host::bcr_refresh(ctx);
      const bool ok = host::bcr_ready(ctx);
      if (ready) ready[s] = ok;
      for (int r = 0; r < nrhs && ok && e == hipSuccess && rc == 0; ++r) {
        if (rhs && x) {
          note(hipMemcpy(host::bcr_rhs(ctx), rhs + (size_t)n * r, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
          if (e == hipSuccess) rc = host::bcr_solve(ctx, nullptr, nullptr, ctx->stream);
          note(hipGetLastError());
          note(hipStreamSynchronize(ctx->stream));
          note(hipMemcpy(x + (size_t)n * (r + (size_t)nrhs * s), host::bcr_sol(ctx), (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        }
        if (rc4 && xc4 && rc == 0) {
          note(hipMemcpy(drc, rc4 + 4 * (size_t)nc * r, 4 * (size_t)nc * sizeof(float), hipMemcpyHostToDevice));
          note(hipMemcpy(dxc, xc4 + 4 * (size_t)nc * (r + (size_t)nrhs * s), 4 * (size_t)nc * sizeof(float), hipMemcpyHostToDevice));
          if (e == hipSuccess) rc = host::bcr_solve(ctx, drc, dxc, ctx->stream);
          note(hipGetLastError());
          note(hipStreamSynchronize(ctx->stream));
          note(hipMemcpy(xc4 + 4 * (size_t)nc * (r + (size_t)nrhs * s), dxc, 4 * (size_t)nc * sizeof(float), hipMemcpyDeviceToHost));
        }
      }
    }
    if (arena32 && cap32 >= (int64_t)d->arena32.n && e == hipSuccess)
      note(hipMemcpy(arena32, d->arena32.p, d->arena32.n * sizeof(float), hipMemcpyDeviceToHost));
    if (tasks && cap_tasks >= (int64_t)d->tasks.n && e == hipSuccess) {
      std::vector<BcrTask> ht(d->tasks.n);
      std::vector<BcrTile> hl(d->tiles.n);
      note(hipMemcpy(ht.data(), d->tasks.p, ht.size() * sizeof(BcrTask), hipMemcpyDeviceToHost));
      note(hipMemcpy(hl.data(), d->tiles.p, hl.size() * sizeof(BcrTile), hipMemcpyDeviceToHost));
      std::vector<int64_t> lev(ht.size(), -1), kind(ht.size(), -1);
      auto tag = [&](const BcrRange& r, int64_t l, int64_t k) {
        for (int64_t t = r.first; t < r.first + r.count; ++t) { lev[hl[t].task] = l; kind[hl[t].task] = k; }
      };
      for (size_t l = 0; l < d->levels.size(); ++l) { tag(d->levels[l].fwd, (int64_t)l, 0); tag(d->levels[l].bwd, (int64_t)l, 1); }
      tag(d->top_task, (int64_t)d->levels.size(), 2);
      for (size_t t = 0; t < ht.size(); ++t) {
        int64_t* q = tasks + 16 * t;
        q[0] = ht[t].w; q[1] = ht[t].rows; q[2] = ht[t].ldw; q[3] = ht[t].out; q[4] = ht[t].nseg;
        for (int k = 0; k < 3; ++k) { q[5 + 3 * k] = ht[t].seg[k].off; q[6 + 3 * k] = ht[t].seg[k].len; q[7 + 3 * k] = ht[t].seg[k].src; }
        q[14] = lev[t]; q[15] = kind[t];
      }
    }
  }
  if (drc) (void)hipFree(drc);
  if (dxc) (void)hipFree(dxc);
  const std::string err = ctx->err;
  delete ctx;
  if (e != hipSuccess) { g_err = std::string("shim_bcr_run: ") + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")"; return 1; }
  if (rc != 0) { g_err = "shim_bcr_run: " + err; return rc; }
  return 0;
}

// ---- fsi_block.hip: field split, Schur complement and the pressure step (tests/test_gpu_block_kernels.py) --------------------
// Every OUTPUT array of the entries below is SHIM_TAIL elements longer than the launch needs: the caller fills the tail with a
// sentinel, the shim uploads and returns it with the rest, and a kernel that writes past its end shows there.
static constexpr size_t SHIM_TAIL = 8;
int shim_tail() { return (int)SHIM_TAIL; }
// launch_block_structure (k_b3_structure, k_vp_structure, k_pv_structure): rowptr3, rowptr_vp [3 N2 + 1], cols3 [9 pairs],
// diagpos3 [3 N2], cols_vp [3 ppairs], cols_pv [rowptr_pv[V]]; rowptr_pv [V + 1] is an input
int shim_block_structure(int64_t N2, int64_t V, const int64_t* nadj_ptr, const int32_t* nadj, const int64_t* padj_ptr, const int32_t* padj,
                         const int32_t* vrank, int64_t* rowptr3, int32_t* cols3, int64_t* diagpos3, int64_t* rowptr_vp, int32_t* cols_vp,
                         const int64_t* rowptr_pv, int32_t* cols_pv) {
  Call c;
  const int64_t np = nadj_ptr[N2], pp = padj_ptr[N2];
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const int64_t* dpp = c.in(padj_ptr, (size_t)N2 + 1);
  const int32_t* dpa = c.in(padj, (size_t)pp);
  const int32_t* dvr = c.in(vrank, (size_t)V);
  int64_t* dr3 = c.io(rowptr3, (size_t)(3 * N2 + 1) + SHIM_TAIL);
  int32_t* dc3 = c.io(cols3, (size_t)(9 * np) + SHIM_TAIL);
  int64_t* dd3 = c.io(diagpos3, (size_t)(3 * N2) + SHIM_TAIL);
  int64_t* drvp = c.io(rowptr_vp, (size_t)(3 * N2 + 1) + SHIM_TAIL);
  int32_t* dcvp = c.io(cols_vp, (size_t)(3 * pp) + SHIM_TAIL);
  const int64_t* drpv = c.in(rowptr_pv, (size_t)V + 1);
  int32_t* dcpv = c.io(cols_pv, (size_t)rowptr_pv[V] + SHIM_TAIL);
  SHIM_RUN(c, "launch_block_structure",
           launch_block_structure(c.st, N2, V, dnp, dn, dpp, dpa, dvr, dr3, dc3, dd3, drvp, dcvp, drpv, dcpv));
}
// A: the monolithic values on rowptr [6 N2 + V + 1]; Add, Adv, Avv [9 pairs], Avp [3 ppairs], Apv [rowptr_pv[V]], App [rowptr_pp[V]]
int shim_extract_blocks(int64_t N2, int64_t V, double ktheta, const int64_t* rowptr, const double* A, const int64_t* nadj_ptr,
                        const int32_t* nadj, const int64_t* padj_ptr, const int32_t* vrank, const int32_t* node_solid,
                        const int64_t* rowptr3, const int64_t* rowptr_vp, const int64_t* rowptr_pv, const int64_t* rowptr_pp, double* Add,
                        double* Adv, double* Avv, double* Avp, double* Apv, double* App) {
  Call c;
  const int64_t n = 6 * N2 + V, np = nadj_ptr[N2], pp = padj_ptr[N2];
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const double* dA = c.in(A, (size_t)rowptr[n]);
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const int64_t* dpp = c.in(padj_ptr, (size_t)N2 + 1);
  const int32_t* dvr = c.in(vrank, (size_t)V);
  const int32_t* dso = c.in(node_solid, (size_t)N2);
  const int64_t* dr3 = c.in(rowptr3, (size_t)(3 * N2 + 1));
  const int64_t* drvp = c.in(rowptr_vp, (size_t)(3 * N2 + 1));
  const int64_t* drpv = c.in(rowptr_pv, (size_t)V + 1);
  const int64_t* drpp = c.in(rowptr_pp, (size_t)V + 1);
  double* dAdd = c.io(Add, (size_t)(9 * np) + SHIM_TAIL);
  double* dAdv = c.io(Adv, (size_t)(9 * np) + SHIM_TAIL);
  double* dAvv = c.io(Avv, (size_t)(9 * np) + SHIM_TAIL);
  double* dAvp = c.io(Avp, (size_t)(3 * pp) + SHIM_TAIL);
  double* dApv = c.io(Apv, (size_t)rowptr_pv[V] + SHIM_TAIL);
  double* dApp = c.io(App, (size_t)rowptr_pp[V] + SHIM_TAIL);
  SHIM_RUN(c, "launch_extract_blocks",
           launch_extract_blocks(c.st, N2, V, ktheta, drp, dA, dnp, dn, dpp, dvr, dso, dr3, drvp, drpv, drpp, dAdd, dAdv, dAvv, dAvp,
                                 dApv, dApp));
}
// vals [9 pairs] on rowptr3; db [3 pairs]; flags [4]
int shim_extract_db(int64_t N2, const int64_t* nadj_ptr, const int64_t* rowptr3, const double* vals, double* db, int32_t* flags,
                    int check) {
  Call c;
  const int64_t np = nadj_ptr[N2];
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int64_t* dr3 = c.in(rowptr3, (size_t)(3 * N2 + 1));
  const double* dv = c.in(vals, (size_t)(9 * np));
  double* ddb = c.io(db, (size_t)(3 * np) + SHIM_TAIL);
  int32_t* df = c.io(flags, 4);
  SHIM_RUN(c, "launch_extract_db", launch_extract_db(c.st, N2, np, dnp, dr3, dv, ddb, df, check));
}
// db [3 pairs]; chat [pairs]; rowflag [3 N2]; flags [4]
int shim_extract_chat(int64_t N2, const int64_t* nadj_ptr, const int32_t* nadj, const double* db, float* chat, uint8_t* rowflag,
                      int32_t* flags) {
  Call c;
  const int64_t np = nadj_ptr[N2];
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const double* ddb = c.in(db, (size_t)(3 * np));
  float* dc = c.io(chat, (size_t)np + SHIM_TAIL);
  uint8_t* drf = c.io(rowflag, (size_t)(3 * N2) + SHIM_TAIL);
  int32_t* df = c.io(flags, 4);
  SHIM_RUN(c, "launch_extract_chat", launch_extract_chat(c.st, N2, dnp, dn, ddb, dc, drf, df));
}
int shim_db_rowmask(int64_t N2, const int64_t* nadj_ptr, const double* db, uint8_t* rowmask) {
  Call c;
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const double* ddb = c.in(db, (size_t)(3 * nadj_ptr[N2]));
  uint8_t* dm = c.io(rowmask, (size_t)N2 + SHIM_TAIL);
  SHIM_RUN(c, "launch_db_rowmask", launch_db_rowmask(c.st, N2, dnp, ddb, dm));
}
int shim_mask_outside(int64_t N2, const uint8_t* rowmask, const int32_t* node_set, int32_t* flags) {
  Call c;
  const uint8_t* dm = c.in(rowmask, (size_t)N2);
  const int32_t* ds = c.in(node_set, (size_t)N2);
  int32_t* df = c.io(flags, 4);
  SHIM_RUN(c, "launch_mask_outside", launch_mask_outside(c.st, N2, dm, ds, df));
}
int shim_to_f32(int64_t n, const double* a, float* b) {
  Call c;
  const double* da = c.in(a, (size_t)n);
  float* db = c.io(b, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_to_f32", launch_to_f32(c.st, n, da, db));
}
int shim_gather_vals(int64_t n, const int64_t* pos, const double* src, int64_t nsrc, double* dst) {
  for (int64_t i = 0; i < n; ++i)
    if (pos[i] < 0 || pos[i] >= nsrc) { g_err = "shim_gather_vals: position " + std::to_string(i) + " outside src"; return 3; }
  Call c;
  const int64_t* dp = c.in(pos, (size_t)n);
  const double* ds = c.in(src, (size_t)nsrc);
  double* dd = c.io(dst, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_gather_vals", launch_gather_vals(c.st, n, dp, ds, dd));
}
// sb_row [nb] (row index < nS into sb_stride [nS]), sb_src [nb]; Avv [nA]; vals [9 nb]
int shim_sb_gather(int64_t nb, int64_t nS, const int32_t* sb_row, const int64_t* sb_src, const int32_t* sb_stride, const double* Avv,
                   int64_t nA, float* vals) {
  for (int64_t b = 0; b < nb; ++b) {
    const bool ok = sb_row[b] >= 0 && sb_row[b] < nS && sb_src[b] >= 0 && sb_stride[sb_row[b]] >= 0 &&
                    sb_src[b] + 2 * (int64_t)sb_stride[sb_row[b]] + 2 < nA;
    if (!ok) { g_err = "shim_sb_gather: block " + std::to_string(b) + " reads outside Avv"; return 3; }
  }
  Call c;
  const int32_t* dr = c.in(sb_row, (size_t)nb);
  const int64_t* ds = c.in(sb_src, (size_t)nb);
  const int32_t* dst = c.in(sb_stride, (size_t)nS);
  const double* dA = c.in(Avv, (size_t)nA);
  float* dv = c.io(vals, (size_t)(9 * nb) + SHIM_TAIL);
  SHIM_RUN(c, "launch_sb_gather", launch_sb_gather(c.st, nb, dr, ds, dst, dA, dv));
}
// S [s_rowptr[V]]; flags [4]; the block arrays as launch_block_structure / launch_extract_blocks lay them out
int shim_schur_full(int64_t V, int64_t N2, const int64_t* s_rowptr, const int32_t* s_cols, const int32_t* vrank, const int64_t* nadj_ptr,
                    const int32_t* nadj, const int64_t* padj_ptr, const int32_t* padj, const int64_t* rowptr_pv, const double* Apv,
                    const int64_t* rowptr_pp, const double* App, const int64_t* rowptr_vp, const double* Avp, const int64_t* diagpos3,
                    const double* Avv, double* S, int32_t* flags) {
  Call c;
  const int64_t np = nadj_ptr[N2], pp = padj_ptr[N2];
  const int64_t* dsr = c.in(s_rowptr, (size_t)V + 1);
  const int32_t* dsc = c.in(s_cols, (size_t)s_rowptr[V]);
  const int32_t* dvr = c.in(vrank, (size_t)V);
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const int64_t* dpp = c.in(padj_ptr, (size_t)N2 + 1);
  const int32_t* dpa = c.in(padj, (size_t)pp);
  const int64_t* drpv = c.in(rowptr_pv, (size_t)V + 1);
  const double* dApv = c.in(Apv, (size_t)rowptr_pv[V]);
  const int64_t* drpp = c.in(rowptr_pp, (size_t)V + 1);
  const double* dApp = c.in(App, (size_t)rowptr_pp[V]);
  const int64_t* drvp = c.in(rowptr_vp, (size_t)(3 * N2 + 1));
  const double* dAvp = c.in(Avp, (size_t)(3 * pp));
  const int64_t* dd3 = c.in(diagpos3, (size_t)(3 * N2));
  const double* dAvv = c.in(Avv, (size_t)(9 * np));
  double* dS = c.io(S, (size_t)s_rowptr[V] + SHIM_TAIL);
  int32_t* df = c.io(flags, 4);
  SHIM_RUN(c, "launch_schur_full",
           launch_schur_full(c.st, V, dsr, dsc, dvr, dnp, dn, dpp, dpa, drpv, dApv, drpp, dApp, drvp, dAvp, dd3, dAvv, dS, df));
}
// apv [rowptr_pv[V]] floats, w [3 N2], c [V], y [V]
int shim_pres_rhs32(int64_t V, int64_t N2, const int32_t* vrank, const int64_t* nadj_ptr, const int32_t* nadj, const int64_t* rowptr_pv,
                    const float* apv, const double* w, const double* cc, double* y) {
  Call c;
  const int32_t* dvr = c.in(vrank, (size_t)V);
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)nadj_ptr[N2]);
  const int64_t* drpv = c.in(rowptr_pv, (size_t)V + 1);
  const float* da = c.in(apv, (size_t)rowptr_pv[V]);
  const double* dw = c.in(w, (size_t)(3 * N2));
  const double* dc = c.in(cc, (size_t)V);
  double* dy = c.io(y, (size_t)V + SHIM_TAIL);
  SHIM_RUN(c, "launch_pres_rhs32", launch_pres_rhs32(c.st, V, dvr, dnp, dn, drpv, da, dw, dc, dy));
}
// avp [3 ppairs] floats, dp [V], dinv [3 N2], vs [3 N2] (may be null), dv [3 N2]
int shim_vel_correct32(int64_t N2, int64_t V, const int64_t* padj_ptr, const int32_t* padj, const float* avp, const double* dp,
                       const double* dinv, const double* vs, double* dv) {
  Call c;
  const int64_t pp = padj_ptr[N2];
  const int64_t* dpp = c.in(padj_ptr, (size_t)N2 + 1);
  const int32_t* dpa = c.in(padj, (size_t)pp);
  const float* da = c.in(avp, (size_t)(3 * pp));
  const double* ddp = c.in(dp, (size_t)V);
  const double* ddi = c.in(dinv, (size_t)(3 * N2));
  const double* dvs = c.in(vs, (size_t)(3 * N2));
  double* ddv = c.io(dv, (size_t)(3 * N2) + SHIM_TAIL);
  SHIM_RUN(c, "launch_vel_correct32", launch_vel_correct32(c.st, N2, dpp, dpa, da, ddp, ddi, dvs, ddv));
}
// CSR (rowptr [n3 + 1], cols, vals) x dp [ndp]; Avv [nA] read at diagpos3 [n3] when dinv [n3] is null; vs [n3] may be null
int shim_vel_correct(int64_t n3, const int64_t* rowptr, const int32_t* cols, const double* vals, const double* dp, int64_t ndp,
                     const int64_t* diagpos3, const double* Avv, int64_t nA, const double* vs, double* dv, const double* dinv) {
  Call c;
  const int64_t* drp = c.in(rowptr, (size_t)n3 + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n3]);
  const double* dvl = c.in(vals, (size_t)rowptr[n3]);
  const double* ddp = c.in(dp, (size_t)ndp);
  const int64_t* dd3 = c.in(diagpos3, (size_t)n3);
  const double* dA = c.in(Avv, (size_t)nA);
  const double* dvs = c.in(vs, (size_t)n3);
  double* ddv = c.io(dv, (size_t)n3 + SHIM_TAIL);
  const double* ddi = c.in(dinv, (size_t)n3);
  SHIM_RUN(c, "launch_vel_correct", launch_vel_correct(c.st, n3, drp, dc, dvl, ddp, dd3, dA, dvs, ddv, ddi));
}
// y [V] = alpha App x + beta Apv w + gamma c; x [V], w [nw], c [V] (x, w, c may be null where their factor is zero)
int shim_pres_rows(int64_t V, const int64_t* rowptr_pp, const int32_t* cols_pp, const double* App, const double* x, double alpha,
                   const int64_t* rowptr_pv, const int32_t* cols_pv, const double* Apv, const double* w, int64_t nw, double beta,
                   const double* cc, double gamma, double* y) {
  Call c;
  const int64_t* drpp = c.in(rowptr_pp, (size_t)V + 1);
  const int32_t* dcpp = c.in(cols_pp, (size_t)rowptr_pp[V]);
  const double* dApp = c.in(App, (size_t)rowptr_pp[V]);
  const double* dx = c.in(x, (size_t)V);
  const int64_t* drpv = c.in(rowptr_pv, (size_t)V + 1);
  const int32_t* dcpv = c.in(cols_pv, (size_t)rowptr_pv[V]);
  const double* dApv = c.in(Apv, (size_t)rowptr_pv[V]);
  const double* dw = c.in(w, (size_t)nw);
  const double* dc = c.in(cc, (size_t)V);
  double* dy = c.io(y, (size_t)V + SHIM_TAIL);
  SHIM_RUN(c, "launch_pres_rows",
           launch_pres_rows(c.st, V, drpp, dcpp, dApp, dx, alpha, drpv, dcpv, dApv, dw, beta, dc, gamma, dy));
}
// mask [n] may be null; A [nA] read at diagpos [n]; x, r, d [n]
int shim_cheb_init(int64_t n, const double* mask, const double* rhs, const int64_t* diagpos, const double* A, int64_t nA,
                   double inv_theta, double* x, double* r, double* d) {
  Call c;
  const double* dm = c.in(mask, (size_t)n);
  const double* drh = c.in(rhs, (size_t)n);
  const int64_t* ddp = c.in(diagpos, (size_t)n);
  const double* dA = c.in(A, (size_t)nA);
  double* dx = c.io(x, (size_t)n + SHIM_TAIL);
  double* dr = c.io(r, (size_t)n + SHIM_TAIL);
  double* dd = c.io(d, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_cheb_init", launch_cheb_init(c.st, n, dm, drh, ddp, dA, inv_theta, dx, dr, dd));
}
int shim_cheb_step(int64_t n, const double* mask, const double* t, const int64_t* diagpos, const double* A, int64_t nA, double c1,
                   double c2, double* x, double* r, double* d) {
  Call c;
  const double* dm = c.in(mask, (size_t)n);
  const double* dt = c.in(t, (size_t)n);
  const int64_t* ddp = c.in(diagpos, (size_t)n);
  const double* dA = c.in(A, (size_t)nA);
  double* dx = c.io(x, (size_t)n + SHIM_TAIL);
  double* dr = c.io(r, (size_t)n + SHIM_TAIL);
  double* dd = c.io(d, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_cheb_step", launch_cheb_step(c.st, n, dm, dt, ddp, dA, c1, c2, dx, dr, dd));
}
// list [nl] node ranks < N2; db [3 pairs]; rowmask [N2] may be null; x, y [3 N2] (y in place)
int shim_db_rows_sub(int64_t nl, int64_t N2, const int32_t* list, const int64_t* nadj_ptr, const int32_t* nadj, const double* db,
                     const uint8_t* rowmask, const double* x, double* y) {
  for (int64_t i = 0; i < nl; ++i)
    if (list[i] < 0 || list[i] >= N2) { g_err = "shim_db_rows_sub: list entry " + std::to_string(i) + " is no node"; return 3; }
  Call c;
  const int64_t np = nadj_ptr[N2];
  const int32_t* dl = c.in(list, (size_t)nl);
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const double* ddb = c.in(db, (size_t)(3 * np));
  const uint8_t* dm = c.in(rowmask, (size_t)N2);
  const double* dx = c.in(x, (size_t)(3 * N2));
  double* dy = c.io(y, (size_t)(3 * N2) + SHIM_TAIL);
  SHIM_RUN(c, "launch_db_rows_sub", launch_db_rows_sub(c.st, nl, dl, dnp, dn, ddb, dm, dx, dy));
}
int shim_spmv_db(int64_t N2, const int64_t* nadj_ptr, const int32_t* nadj, const double* db, const double* x, double* y,
                 const uint8_t* rowmask) {
  Call c;
  const int64_t np = nadj_ptr[N2];
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  const int32_t* dn = c.in(nadj, (size_t)np);
  const double* ddb = c.in(db, (size_t)(3 * np));
  const double* dx = c.in(x, (size_t)(3 * N2));
  double* dy = c.io(y, (size_t)(3 * N2) + SHIM_TAIL);
  const uint8_t* dm = c.in(rowmask, (size_t)N2);
  SHIM_RUN(c, "launch_spmv_db", launch_spmv_db(c.st, N2, dnp, dn, ddb, dx, dy, dm));
}
// y [n] = b - A x on a CSR matrix with columns < nx
int shim_residual_csr(int64_t n, const int64_t* rowptr, const int32_t* cols, const double* vals, const double* x, int64_t nx,
                      const double* b, double* y) {
  Call c;
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n]);
  const double* dv = c.in(vals, (size_t)rowptr[n]);
  const double* dx = c.in(x, (size_t)nx);
  const double* db = c.in(b, (size_t)n);
  double* dy = c.io(y, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_residual_csr", launch_residual_csr(c.st, n, drp, dc, dv, dx, db, dy));
}
// rows [nrows] < ny; ptr [nrows + 1]; col, src [ptr[nrows]] (col < nx, src < nvals); b, y [ny] (y in place)
int shim_residual_rows(int64_t nrows, const int32_t* rows, const int64_t* ptr, const int32_t* col, const int64_t* src, const double* vals,
                       int64_t nvals, const double* x, int64_t nx, const double* b, double* y, int64_t ny) {
  for (int64_t i = 0; i < nrows; ++i)
    if (rows[i] < 0 || rows[i] >= ny) { g_err = "shim_residual_rows: row " + std::to_string(i) + " outside y"; return 3; }
  const int64_t ne = nrows > 0 ? ptr[nrows] : 0;
  for (int64_t t = 0; t < ne; ++t)
    if (col[t] < 0 || col[t] >= nx || src[t] < 0 || src[t] >= nvals) { g_err = "shim_residual_rows: entry " + std::to_string(t) + " out of range"; return 3; }
  Call c;
  const int32_t* dr = c.in(rows, (size_t)nrows);
  const int64_t* dp = c.in(ptr, (size_t)nrows + 1);
  const int32_t* dc = c.in(col, (size_t)ne);
  const int64_t* ds = c.in(src, (size_t)ne);
  const double* dv = c.in(vals, (size_t)nvals);
  const double* dx = c.in(x, (size_t)nx);
  const double* db = c.in(b, (size_t)ny);
  double* dy = c.io(y, (size_t)ny + SHIM_TAIL);
  SHIM_RUN(c, "launch_residual_rows", launch_residual_rows(c.st, nrows, dr, dp, dc, ds, dv, dx, db, dy));
}
// r [6 N2 + V] -> rd, rv [3 N2], rp [V]
int shim_split(int64_t N2, int64_t V, const double* r, double* rd, double* rv, double* rp) {
  Call c;
  const double* dr = c.in(r, (size_t)(6 * N2 + V));
  double* drd = c.io(rd, (size_t)(3 * N2) + SHIM_TAIL);
  double* drv = c.io(rv, (size_t)(3 * N2) + SHIM_TAIL);
  double* drp = c.io(rp, (size_t)V + SHIM_TAIL);
  SHIM_RUN(c, "launch_split", launch_split(c.st, N2, V, dr, drd, drv, drp));
}
int shim_merge(int64_t N2, int64_t V, const double* zd, const double* zv, const double* zp, double* z) {
  Call c;
  const double* dzd = c.in(zd, (size_t)(3 * N2));
  const double* dzv = c.in(zv, (size_t)(3 * N2));
  const double* dzp = c.in(zp, (size_t)V);
  double* dz = c.io(z, (size_t)(6 * N2 + V) + SHIM_TAIL);
  SHIM_RUN(c, "launch_merge", launch_merge(c.st, N2, V, dzd, dzv, dzp, dz));
}
int shim_merge_f32d(int64_t N2, int64_t V, const float* xd4, const double* zv, const double* zp, double* z) {
  Call c;
  const float* dxd = c.in(xd4, (size_t)(4 * N2));
  const double* dzv = c.in(zv, (size_t)(3 * N2));
  const double* dzp = c.in(zp, (size_t)V);
  double* dz = c.io(z, (size_t)(6 * N2 + V) + SHIM_TAIL);
  SHIM_RUN(c, "launch_merge_f32d", launch_merge_f32d(c.st, N2, V, dxd, dzv, dzp, dz));
}
// a [3 nn]; scale4 [4 nn] may be null; dinv4, x, r, d [4 nn]
int shim_pad_init_f32(int64_t nn, const double* a, const float* scale4, const float* dinv4, float inv_theta, float* x, float* r,
                      float* d) {
  Call c;
  const double* da = c.in(a, (size_t)(3 * nn));
  const float* ds = c.in(scale4, (size_t)(4 * nn));
  const float* ddi = c.in(dinv4, (size_t)(4 * nn));
  float* dx = c.io(x, (size_t)(4 * nn) + SHIM_TAIL);
  float* dr = c.io(r, (size_t)(4 * nn) + SHIM_TAIL);
  float* dd = c.io(d, (size_t)(4 * nn) + SHIM_TAIL);
  SHIM_RUN(c, "launch_pad_init_f32", launch_pad_init_f32(c.st, nn, da, ds, ddi, inv_theta, dx, dr, dd));
}
int shim_pad_to_f32(int64_t nn, const double* a, const float* scale4, float* b) {
  Call c;
  const double* da = c.in(a, (size_t)(3 * nn));
  const float* ds = c.in(scale4, (size_t)(4 * nn));
  float* db = c.io(b, (size_t)(4 * nn) + SHIM_TAIL);
  SHIM_RUN(c, "launch_pad_to_f32", launch_pad_to_f32(c.st, nn, da, ds, db));
}
int shim_unpad_from_f32(int64_t nn, const float* a, double* b) {
  Call c;
  const float* da = c.in(a, (size_t)(4 * nn));
  double* db = c.io(b, (size_t)(3 * nn) + SHIM_TAIL);
  SHIM_RUN(c, "launch_unpad_from_f32", launch_unpad_from_f32(c.st, nn, da, db));
}
int shim_mask_ripple(int64_t n, const double* mask, double* x) {
  Call c;
  const double* dm = c.in(mask, (size_t)n);
  double* dx = c.io(x, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_mask_ripple", launch_mask_ripple(c.st, n, dm, dx));
}
// y [n] in place; A [nA] read at diagpos [n]
int shim_mask_scale(int64_t n, const double* mask, const int64_t* diagpos, const double* A, int64_t nA, double* y) {
  Call c;
  const double* dm = c.in(mask, (size_t)n);
  const int64_t* ddp = c.in(diagpos, (size_t)n);
  const double* dA = c.in(A, (size_t)nA);
  double* dy = c.io(y, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_mask_scale", launch_mask_scale(c.st, n, dm, ddp, dA, dy));
}

// ---- fsi_solver.hip: multicolour ILU(0) and its triangular solves (tests/test_gpu_ilu_kernels.py) ---------------------------
// Levels: nlevels x (level_first, level_ngroups, level_group_rows).  The matrix is checked on the host before anything is
// launched, because the kernels trust it: levels inside 0 .. n, columns inside 0 .. n, every row's diagpos inside the row.
// Status 3 (nothing launched) otherwise.
namespace {
int levels_checked(const char* who, int64_t n, int nlevels, const int64_t* first, const int64_t* ngroups, const int32_t* group_rows,
                   const int64_t* rowptr, const int32_t* cols, const int64_t* diagpos, std::vector<Level>& levels) {
  auto bad = [&](const std::string& what) { g_err = std::string(who) + ": " + what; return 3; };
  if (n < 0 || nlevels < 0 || rowptr[0] != 0) return bad("bad sizes");
  for (int64_t i = 0; i < n; ++i) {
    if (rowptr[i + 1] < rowptr[i]) return bad("rowptr decreases at row " + std::to_string(i));
    if (diagpos[i] < rowptr[i] || diagpos[i] >= rowptr[i + 1]) return bad("row " + std::to_string(i) + " has no diagonal entry inside the row");
    if (cols[diagpos[i]] != i) return bad("diagpos of row " + std::to_string(i) + " is not its diagonal");
  }
  for (int64_t t = 0; t < rowptr[n]; ++t)
    if (cols[t] < 0 || cols[t] >= n) return bad("column outside the matrix at entry " + std::to_string(t));
  levels.clear();
  for (int l = 0; l < nlevels; ++l) {
    if (first[l] < 0 || ngroups[l] < 0 || group_rows[l] < 1 || first[l] + ngroups[l] * group_rows[l] > n)
      return bad("level " + std::to_string(l) + " outside the matrix");
    levels.push_back(Level{first[l], ngroups[l], group_rows[l]});
  }
  return 0;
}
}  // namespace
// LU [rowptr[n]] in place (+ SHIM_TAIL); counters [4] in/out
int shim_ilu0(int64_t n, int nlevels, const int64_t* level_first, const int64_t* level_ngroups, const int32_t* level_group_rows,
              const int64_t* rowptr, const int32_t* cols, const int64_t* diagpos, double* LU, int32_t* counters) {
  std::vector<Level> levels;
  if (const int rc = levels_checked("shim_ilu0", n, nlevels, level_first, level_ngroups, level_group_rows, rowptr, cols, diagpos, levels))
    return rc;
  Call c;
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n]);
  const int64_t* ddp = c.in(diagpos, (size_t)n);
  double* dLU = c.io(LU, (size_t)rowptr[n] + SHIM_TAIL);
  int32_t* dcn = c.io(counters, 4);
  SHIM_RUN(c, "launch_ilu0_levels", launch_ilu0_levels(c.st, levels, drp, dc, ddp, dLU, dcn));
}
// rhs [n]; tmp (the forward result y) and x [n + SHIM_TAIL], both returned
int shim_sptrsv(int64_t n, int nlevels, const int64_t* level_first, const int64_t* level_ngroups, const int32_t* level_group_rows,
                const int64_t* rowptr, const int32_t* cols, const int64_t* diagpos, const double* LU, const double* rhs, double* tmp,
                double* x) {
  std::vector<Level> levels;
  if (const int rc = levels_checked("shim_sptrsv", n, nlevels, level_first, level_ngroups, level_group_rows, rowptr, cols, diagpos, levels))
    return rc;
  Call c;
  const int64_t* drp = c.in(rowptr, (size_t)n + 1);
  const int32_t* dc = c.in(cols, (size_t)rowptr[n]);
  const int64_t* ddp = c.in(diagpos, (size_t)n);
  const double* dLU = c.in(LU, (size_t)rowptr[n]);
  const double* drhs = c.in(rhs, (size_t)n);
  double* dtmp = c.io(tmp, (size_t)n + SHIM_TAIL);
  double* dx = c.io(x, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_sptrsv_levels", launch_sptrsv_levels(c.st, levels, drp, dc, ddp, dLU, drhs, dtmp, dx));
}

// ---- fsi_solver.hip / fsi_block.hip: boundary terms and small vector launchers (tests/test_gpu_vector_kernels.py) ------------
// Outputs of n entries carry SHIM_TAIL sentinels; an indexed target has its own length (nt) and the indices are checked on the
// host first (status 3, nothing launched).
extern "C++" {
namespace {
template <class I>
int indices_checked(const char* who, const I* idx, int64_t n, int64_t nt) {
  for (int64_t i = 0; i < n; ++i)
    if (idx[i] < 0 || (int64_t)idx[i] >= nt) { g_err = std::string(who) + ": index " + std::to_string(i) + " outside the target"; return 3; }
  return 0;
}
}  // namespace
}  // extern "C++"
int shim_fill(int64_t n, double v, double* x) {
  Call c;
  double* dx = c.io(x, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_fill", launch_fill(c.st, dx, n, v));
}
int shim_copy(int64_t n, const double* s, double* d) {
  Call c;
  const double* ds = c.in(s, (size_t)n);
  double* dd = c.io(d, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_copy", launch_copy(c.st, dd, ds, n));
}
int shim_axpy(int64_t n, double a, const double* x, double* y) {
  Call c;
  const double* dx = c.in(x, (size_t)n);
  double* dy = c.io(y, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_axpy", launch_axpy(c.st, dy, a, dx, n));
}
int shim_axpby(int64_t n, double a, const double* x, double b, const double* y, double* z) {
  Call c;
  const double* dx = c.in(x, (size_t)n);
  const double* dy = c.in(y, (size_t)n);
  double* dz = c.io(z, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_axpby", launch_axpby(c.st, dz, a, dx, b, dy, n));
}
int shim_scale(int64_t n, double a, double* y) {
  Call c;
  double* dy = c.io(y, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_scale", launch_scale(c.st, dy, a, n));
}
int shim_mul(int64_t n, const double* x, const double* y, double* z) {
  Call c;
  const double* dx = c.in(x, (size_t)n);
  const double* dy = c.in(y, (size_t)n);
  double* dz = c.io(z, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_mul", launch_mul(c.st, dz, dx, dy, n));
}
int shim_div(int64_t n, const double* x, const double* y, double* z) {
  Call c;
  const double* dx = c.in(x, (size_t)n);
  const double* dy = c.in(y, (size_t)n);
  double* dz = c.io(z, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_div", launch_div(c.st, dz, dx, dy, n));
}
int shim_negate(int64_t n, const double* F, double* b) {
  Call c;
  const double* dF = c.in(F, (size_t)n);
  double* db = c.io(b, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_negate", launch_negate(c.st, db, dF, n));
}
// d[i] = s[idx[i]]: s [ns], d [n + SHIM_TAIL]
int shim_gather(int64_t n, const double* s, int64_t ns, const int32_t* idx, double* d) {
  if (const int rc = indices_checked("shim_gather", idx, n, ns)) return rc;
  Call c;
  const double* ds = c.in(s, (size_t)ns);
  const int32_t* di = c.in(idx, (size_t)n);
  double* dd = c.io(d, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_gather", launch_gather(c.st, dd, ds, di, n));
}
// d[idx[i]] = s[i]: s [n], d [nd] in place
int shim_scatter(int64_t n, const double* s, const int32_t* idx, double* d, int64_t nd) {
  if (const int rc = indices_checked("shim_scatter", idx, n, nd)) return rc;
  Call c;
  const double* ds = c.in(s, (size_t)n);
  const int32_t* di = c.in(idx, (size_t)n);
  double* dd = c.io(d, (size_t)nd);
  SHIM_RUN(c, "launch_scatter", launch_scatter(c.st, dd, ds, di, n));
}
// comp[3 k + i] = full[3 snode[k] + i]: full [3 nnodes], comp [3 nS + SHIM_TAIL]
int shim_gather3(int64_t nS, int64_t nnodes, const int32_t* snode, const double* full, double* comp) {
  if (const int rc = indices_checked("shim_gather3", snode, nS, nnodes)) return rc;
  Call c;
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const double* dfu = c.in(full, (size_t)(3 * nnodes));
  double* dco = c.io(comp, (size_t)(3 * nS) + SHIM_TAIL);
  SHIM_RUN(c, "launch_gather3", launch_gather3(c.st, nS, dsn, dfu, dco));
}
// full [3 nnodes] in place
int shim_scatter3(int64_t nS, int64_t nnodes, const int32_t* snode, const double* comp, double* full) {
  if (const int rc = indices_checked("shim_scatter3", snode, nS, nnodes)) return rc;
  Call c;
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const double* dco = c.in(comp, (size_t)(3 * nS));
  double* dfu = c.io(full, (size_t)(3 * nnodes));
  SHIM_RUN(c, "launch_scatter3", launch_scatter3(c.st, nS, dsn, dco, dfu));
}
int shim_round_to_f32(int64_t n, const double* a, float* b) {
  Call c;
  const double* da = c.in(a, (size_t)n);
  float* db = c.io(b, (size_t)n + SHIM_TAIL);
  SHIM_RUN(c, "launch_round_to_f32", launch_round_to_f32(c.st, n, da, db));
}
// y[idx[i]] += a coef[i]: y [ny] in place
int shim_add_indexed(int64_t n, const int32_t* idx, const double* coef, double a, double* y, int64_t ny) {
  if (const int rc = indices_checked("shim_add_indexed", idx, n, ny)) return rc;
  Call c;
  const int32_t* di = c.in(idx, (size_t)n);
  const double* dco = c.in(coef, (size_t)n);
  double* dy = c.io(y, (size_t)ny);
  SHIM_RUN(c, "launch_add_indexed", launch_add_indexed(c.st, dy, di, dco, a, n));
}
// vals[pos[i]] += a v[i]: vals [nvals] in place
int shim_add_at(int64_t n, const int64_t* pos, const double* v, double a, double* vals, int64_t nvals) {
  if (const int rc = indices_checked("shim_add_at", pos, n, nvals)) return rc;
  Call c;
  const int64_t* dp = c.in(pos, (size_t)n);
  const double* dv = c.in(v, (size_t)n);
  double* dvals = c.io(vals, (size_t)nvals);
  SHIM_RUN(c, "launch_add_at", launch_add_at(c.st, dvals, dp, dv, a, n));
}
// b[bc[i]] = g[i] - U[bc[i]]: b (in place), U [nu]
int shim_bc_rhs(int64_t n, const int32_t* bc, const double* g, const double* U, double* b, int64_t nu) {
  if (const int rc = indices_checked("shim_bc_rhs", bc, n, nu)) return rc;
  Call c;
  const int32_t* dbc = c.in(bc, (size_t)n);
  const double* dg = c.in(g, (size_t)n);
  const double* dU = c.in(U, (size_t)nu);
  double* db = c.io(b, (size_t)nu);
  SHIM_RUN(c, "launch_bc_rhs", launch_bc_rhs(c.st, db, dU, dbc, dg, n));
}
// U[bc[i]] = g[i]: U [nu] in place
int shim_bc_set(int64_t n, const int32_t* bc, const double* g, double* U, int64_t nu) {
  if (const int rc = indices_checked("shim_bc_set", bc, n, nu)) return rc;
  Call c;
  const int32_t* dbc = c.in(bc, (size_t)n);
  const double* dg = c.in(g, (size_t)n);
  double* dU = c.io(U, (size_t)nu);
  SHIM_RUN(c, "launch_bc_set", launch_bc_set(c.st, dU, dbc, dg, n));
}
// urow [nrows], ptr [nrows + 1], col / val [ptr[nrows]]; U, U1, F (in place) [nu]
int shim_robin_residual(int64_t nrows, const int32_t* urow, const int32_t* ptr, const int32_t* col, const double* val, double th0,
                        double th1, const double* U, const double* U1, double* F, int64_t nu) {
  if (const int rc = indices_checked("shim_robin_residual rows", urow, nrows, nu)) return rc;
  for (int64_t k = 0; k < nrows; ++k)
    if (ptr[k] < 0 || ptr[k + 1] < ptr[k]) { g_err = "shim_robin_residual: ptr decreases at row " + std::to_string(k); return 3; }
  const int64_t ne = ptr[nrows];
  if (const int rc = indices_checked("shim_robin_residual columns", col, ne, nu)) return rc;
  Call c;
  const int32_t* dur = c.in(urow, (size_t)nrows);
  const int32_t* dp = c.in(ptr, (size_t)nrows + 1);
  const int32_t* dcl = c.in(col, (size_t)ne);
  const double* dv = c.in(val, (size_t)ne);
  const double* dU = c.in(U, (size_t)nu);
  const double* dU1 = c.in(U1, (size_t)nu);
  double* dF = c.io(F, (size_t)nu);
  SHIM_RUN(c, "launch_robin_residual", launch_robin_residual(c.st, nrows, dur, dp, dcl, dv, th0, th1, dU, dU1, dF));
}
// x [4 nnodes + SHIM_TAIL]
int shim_f32_ripple4(int64_t nnodes, float* x) {
  Call c;
  float* dx = c.io(x, (size_t)(4 * nnodes) + SHIM_TAIL);
  SHIM_RUN(c, "launch_f32_ripple4", launch_f32_ripple4(c.st, nnodes, dx));
}
// out [1 + SHIM_TAIL]
int shim_f32_sumsq(int64_t n, const float* x, double* out) {
  Call c;
  const float* dx = c.in(x, (size_t)n);
  double* dout = c.io(out, 1 + SHIM_TAIL);
  SHIM_RUN(c, "launch_f32_sumsq", launch_f32_sumsq(c.st, n, dx, dout));
}

// ---- fsi_assembly.hip: the element kernels (tests/test_gpu_element_kernels.py, tests/test_gpu_element_jacobian.py) ------------
// Host arrays throughout, no live context: the basis tables are uploaded by the entry itself.  Every index array is checked on the
// host first (status 3, nothing launched): node ranks against N2, dofs against the state's length, incidences against C, and for the
// Jacobian every position an element entry can be added at against its row of the matrix.  ElemParams as plain arrays: sc [5] =
// (k, th0, th1, delta, alpha), fluid [8][2] = (rho, mu), solid [8][7] = (rho, mu, lam, model, C10, C01, C11).
extern "C++" {
namespace {
ElemParams elem_params(const double* sc, const double* fluid, const double* solid) {
  ElemParams ep;
  ep.sc = Scheme{sc[0], sc[1], sc[2], sc[3], sc[4]};
  for (int r = 0; r < MAX_REGIONS; ++r) {
    ep.fluid[r] = FluidProps{fluid[2 * r], fluid[2 * r + 1]};
    const double* p = solid + 7 * r;
    ep.solid[r] = SolidProps{p[0], p[1], p[2], (int)p[3], p[4], p[5], p[6]};
  }
  return ep;
}
int kinds_checked(const char* who, const int32_t* kind, const int32_t* region, int64_t C) {
  for (int64_t c = 0; c < C; ++c)
    if (kind[c] < 0 || kind[c] > 1 || region[c] < 0 || region[c] >= MAX_REGIONS) {
      g_err = std::string(who) + ": kind / region of cell " + std::to_string(c) + " outside the tables";
      return 3;
    }
  return 0;
}
int ptr_checked(const char* who, const int64_t* ptr, int64_t n) {
  if (ptr[0] != 0) { g_err = std::string(who) + ": pointer array does not start at 0"; return 3; }
  for (int64_t i = 0; i < n; ++i)
    if (ptr[i + 1] < ptr[i]) { g_err = std::string(who) + ": pointer array decreases at " + std::to_string(i); return 3; }
  return 0;
}
// incidences 16 * cell + local index, local index below nloc
int incidences_checked(const char* who, const int32_t* inc, int64_t n, int64_t C, int nloc) {
  for (int64_t i = 0; i < n; ++i)
    if (inc[i] < 0 || (inc[i] >> 4) >= C || (inc[i] & 15) >= nloc) { g_err = std::string(who) + ": incidence " + std::to_string(i) + " outside Re"; return 3; }
  return 0;
}
}  // namespace
}  // extern "C++"
// coords [nv][3], tets [C][4]; geom [10 C + SHIM_TAIL]
int shim_geometry(int64_t C, int64_t nv, const double* coords, const int32_t* tets, double* geom) {
  if (const int rc = indices_checked("shim_geometry", tets, 4 * C, nv)) return rc;
  Call c;
  const double* dx = c.in(coords, (size_t)(3 * nv));
  const int32_t* dt = c.in(tets, (size_t)(4 * C));
  double* dg = c.io(geom, (size_t)(10 * C) + SHIM_TAIL);
  SHIM_RUN(c, "launch_geometry", launch_geometry(c.st, C, dx, dt, dg));
}
// U, U1 [nu]; the node ranks lie below nrank (6 nrank <= nu), the pressure rows below nu.
// Gathered form (Re not null): Re [64 C + SHIM_TAIL] and F [6 N2 + V + SHIM_TAIL] are written, inc_ptr [N2 + 1] / inc and
// pinc_ptr [V + 1] / pinc are the incidence lists the gather sums over (they need not be the mesh's own).
// Atomic form (Re null): F [nu + SHIM_TAIL] in / out, N2, V and the lists unused.
int shim_elem_residual(int64_t C, int64_t nu, int64_t nrank, const double* geom, const int32_t* cell_rank, const int32_t* cell_prow,
                       const int32_t* cell_kind, const int32_t* cell_region, const double* sc, const double* fluid,
                       const double* solid, const double* U, const double* U1, int64_t N2, int64_t V, const int64_t* inc_ptr,
                       const int32_t* inc, const int64_t* pinc_ptr, const int32_t* pinc, double* Re, double* F) {
  if (C < 1 || 6 * nrank > nu) { g_err = "shim_elem_residual: no cells, or node ranks beyond the state"; return 3; }
  if (const int rc = indices_checked("shim_elem_residual ranks", cell_rank, 10 * C, nrank)) return rc;
  if (const int rc = indices_checked("shim_elem_residual pressure rows", cell_prow, 4 * C, nu)) return rc;
  if (const int rc = kinds_checked("shim_elem_residual", cell_kind, cell_region, C)) return rc;
  if (Re) {
    if (N2 < 0 || V < 0 || 6 * N2 + V < 1) { g_err = "shim_elem_residual: nothing to gather"; return 3; }
    if (const int rc = ptr_checked("shim_elem_residual inc_ptr", inc_ptr, N2)) return rc;
    if (const int rc = ptr_checked("shim_elem_residual pinc_ptr", pinc_ptr, V)) return rc;
    if (const int rc = incidences_checked("shim_elem_residual inc", inc, inc_ptr[N2], C, 10)) return rc;
    if (const int rc = incidences_checked("shim_elem_residual pinc", pinc, pinc_ptr[V], C, 4)) return rc;
  }
  Call c;
  c.note(upload_tables());
  ElemArrays ea{};
  ea.geom = c.in(geom, (size_t)(10 * C));
  ea.cell_rank = c.in(cell_rank, (size_t)(10 * C));
  ea.cell_prow = c.in(cell_prow, (size_t)(4 * C));
  ea.cell_kind = c.in(cell_kind, (size_t)C);
  ea.cell_region = c.in(cell_region, (size_t)C);
  const ElemParams ep = elem_params(sc, fluid, solid);
  const double* dU = c.in(U, (size_t)nu);
  const double* dU1 = c.in(U1, (size_t)nu);
  ResidualGather rg;
  double* dF;
  if (Re) {
    rg.Re = c.io(Re, (size_t)(NLOC * C) + SHIM_TAIL);
    rg.N2 = N2; rg.V = V;
    rg.inc_ptr = c.in(inc_ptr, (size_t)N2 + 1);
    rg.inc = c.in(inc, (size_t)inc_ptr[N2]);
    rg.pinc_ptr = c.in(pinc_ptr, (size_t)V + 1);
    rg.pinc = c.in(pinc, (size_t)pinc_ptr[V]);
    dF = c.io(F, (size_t)(6 * N2 + V) + SHIM_TAIL);
  } else {
    dF = c.io(F, (size_t)nu + SHIM_TAIL);
  }
  SHIM_RUN(c, "launch_residual", launch_residual(c.st, C, ea, ep, dU, dU1, dF, rg));
}
// part: PART_LINEAR (1) or PART_NONLINEAR (2).  U, U1 [nu]; rowptr [nu + 1]; nadj_ptr [N2 + 1]; vals [rowptr[nu] + SHIM_TAIL] in / out.
// Colours: cells [ptr[ncolours]] sorted by colour, ptr [ncolours + 1] (host); ncolours == 0: one launch over all cells.
int shim_elem_jacobian(int part, int jac_waves, int jac_mfma, int64_t C, int64_t nu, int64_t N2, const double* geom,
                       const int32_t* cell_dofs, const int32_t* cell_kind, const int32_t* cell_region, const int32_t* cell_rank,
                       const uint16_t* enbr, const uint16_t* epnbr, const double* sc, const double* fluid, const double* solid,
                       const double* U, const double* U1, const int64_t* rowptr, const int64_t* nadj_ptr, int ncolours,
                       const int32_t* cells, const int64_t* ptr, double* vals) {
  if (C < 1 || (part != PART_LINEAR && part != PART_NONLINEAR) || ncolours < 0) { g_err = "shim_elem_jacobian: no cells, or no such part"; return 3; }
  if (const int rc = indices_checked("shim_elem_jacobian dofs", cell_dofs, NLOC * C, nu)) return rc;
  if (const int rc = indices_checked("shim_elem_jacobian ranks", cell_rank, 10 * C, N2)) return rc;
  if (const int rc = kinds_checked("shim_elem_jacobian", cell_kind, cell_region, C)) return rc;
  if (const int rc = ptr_checked("shim_elem_jacobian rowptr", rowptr, nu)) return rc;
  if (const int rc = ptr_checked("shim_elem_jacobian nadj_ptr", nadj_ptr, N2)) return rc;
  // every position the kernels can add at: row i of the element, column j, as k_jacobian computes it
  for (int64_t cl = 0; cl < C; ++cl)
    for (int i = 0; i < NLOC; ++i) {
      const int64_t row = cell_dofs[cl * NLOC + i], r0 = rowptr[row], r1 = rowptr[row + 1];
      const int ra = i < 60 ? i % 10 : i - 60;
      const int32_t rk = cell_rank[cl * 10 + ra];
      const int64_t deg6 = 6 * (nadj_ptr[rk + 1] - nadj_ptr[rk]);
      for (int j = 0; j < NLOC; ++j) {
        const int jf = j < 60 ? j / 30 : 2, jc = j < 60 ? (j % 30) / 10 : 0, jb = j < 60 ? j % 10 : j - 60;
        const int64_t pos = jf < 2 ? r0 + 6 * (int64_t)enbr[cl * 100 + ra * 10 + jb] + 3 * jf + jc : r0 + deg6 + epnbr[cl * 40 + ra * 4 + jb];
        if (pos < r0 || pos >= r1) {
          g_err = "shim_elem_jacobian: entry (" + std::to_string(i) + ", " + std::to_string(j) + ") of cell " + std::to_string(cl) + " outside its row";
          return 3;
        }
      }
    }
  int64_t nlist = 0;
  if (ncolours > 0) {
    if (const int rc = ptr_checked("shim_elem_jacobian colours", ptr, ncolours)) return rc;
    nlist = ptr[ncolours];
    if (const int rc = indices_checked("shim_elem_jacobian colour lists", cells, nlist, C)) return rc;
  }
  Call c;
  c.note(upload_tables());
  ElemArrays ea{};
  ea.geom = c.in(geom, (size_t)(10 * C));
  ea.cell_dofs = c.in(cell_dofs, (size_t)(NLOC * C));
  ea.cell_kind = c.in(cell_kind, (size_t)C);
  ea.cell_region = c.in(cell_region, (size_t)C);
  ea.cell_rank = c.in(cell_rank, (size_t)(10 * C));
  ea.enbr = c.in(enbr, (size_t)(100 * C));
  ea.epnbr = c.in(epnbr, (size_t)(40 * C));
  const ElemParams ep = elem_params(sc, fluid, solid);
  const double* dU = c.in(U, (size_t)nu);
  const double* dU1 = c.in(U1, (size_t)nu);
  const int64_t* drp = c.in(rowptr, (size_t)nu + 1);
  const int64_t* dnp = c.in(nadj_ptr, (size_t)N2 + 1);
  double* dv = c.io(vals, (size_t)rowptr[nu] + SHIM_TAIL);
  CellColours cc;
  cc.ncolours = ncolours;
  if (ncolours > 0) { cc.cells = c.in(cells, (size_t)nlist); cc.ptr = ptr; }
  SHIM_RUN(c, "launch_jacobian", launch_jacobian(c.st, part, C, ea, ep, dU, dU1, drp, dnp, dv, cc, jac_waves, jac_mfma));
}
// X [nu]; out [1 + SHIM_TAIL] = int |d|^2 + |v|^2 + p^2 over the cells
int shim_l2norm(int64_t C, int64_t nu, const double* geom, const int32_t* cell_dofs, const double* X, double* out) {
  if (C < 1) { g_err = "shim_l2norm: no cells"; return 3; }
  if (const int rc = indices_checked("shim_l2norm", cell_dofs, NLOC * C, nu)) return rc;
  Call c;
  c.note(upload_tables());
  ElemArrays ea{};
  ea.geom = c.in(geom, (size_t)(10 * C));
  ea.cell_dofs = c.in(cell_dofs, (size_t)(NLOC * C));
  const double* dX = c.in(X, (size_t)nu);
  std::vector<double> hs(4096 + 16);
  double* part = c.in(hs.data(), hs.size());
  double* dout = c.io(out, 1 + SHIM_TAIL);
  SHIM_RUN(c, "launch_l2norm", launch_l2norm(c.st, C, ea, dX, part, dout));
}
int shim_stat_parts() { return STAT_PARTS; }
// X [nu]; cellvals [2 C + 8 + 4 STAT_PARTS + SHIM_TAIL]: the cell means of |v| [C] and of det(I + grad d) [C], then (sum, min, max
// of the first, min of the second), four unused, and the partials of the reduction's first stage
int shim_cell_stats(int64_t C, int64_t nu, int64_t nrank, const double* geom, const int32_t* cell_rank, const int32_t* cell_prow,
                    const double* X, double* cellvals) {
  if (C < 1 || 6 * nrank > nu) { g_err = "shim_cell_stats: no cells, or node ranks beyond the state"; return 3; }
  if (const int rc = indices_checked("shim_cell_stats ranks", cell_rank, 10 * C, nrank)) return rc;
  if (const int rc = indices_checked("shim_cell_stats pressure rows", cell_prow, 4 * C, nu)) return rc;
  Call c;
  c.note(upload_tables());
  ElemArrays ea{};
  ea.geom = c.in(geom, (size_t)(10 * C));
  ea.cell_rank = c.in(cell_rank, (size_t)(10 * C));
  ea.cell_prow = c.in(cell_prow, (size_t)(4 * C));
  const double* dX = c.in(X, (size_t)nu);
  double* dcv = c.io(cellvals, (size_t)(2 * C + 8 + 4 * STAT_PARTS) + SHIM_TAIL);
  SHIM_RUN(c, "launch_cell_stats", launch_cell_stats(c.st, C, ea, dX, dcv, dcv + 2 * C));
}
// cells [n] (below C), bary [n][4], X [nu]; out [7 n + SHIM_TAIL] = d(3), v(3), p per point
int shim_probe(int64_t n, int64_t C, int64_t nu, const int32_t* cell_dofs, const int32_t* cells, const double* bary, const double* X,
               double* out) {
  if (n < 1) { g_err = "shim_probe: no points"; return 3; }
  if (const int rc = indices_checked("shim_probe dofs", cell_dofs, NLOC * C, nu)) return rc;
  if (const int rc = indices_checked("shim_probe cells", cells, n, C)) return rc;
  Call c;
  ElemArrays ea{};
  ea.cell_dofs = c.in(cell_dofs, (size_t)(NLOC * C));
  const int32_t* dc = c.in(cells, (size_t)n);
  const double* db = c.in(bary, (size_t)(4 * n));
  const double* dX = c.in(X, (size_t)nu);
  double* dout = c.io(out, (size_t)(7 * n) + SHIM_TAIL);
  SHIM_RUN(c, "launch_probe", launch_probe(c.st, n, ea, dc, db, dX, dout));
}

// ---- fsi_post.hip, fsi_hemo.hip, fsi_stress.hip: wall shear stress, hemodynamic sums and indices, solid stress / strain and
// principal values, one cell (or dof) at a time (tests/test_gpu_post_cell_kernels.py; references in tests/post_cells.py) --------------
// Host arrays throughout, no live context.  The cell arrays are those of a case of C cells (geom [C][10], cell_dofs [C][64],
// cell_region [C]), the launch runs over the list cells [ncell] (any order, repeats allowed).  Every entry uploads the tables its
// kernel reads from arrays the caller passes: upload_post_tables (which fills the copies of fsi_stress.hip too) with the Keast-24
// weights qw [24], dN [24][10][3] and L [24][4]; hemo_upload_tables with the triangle rule tw [12], tl [12][3].  ElemParams as for the
// element kernels.  Every index array is checked on the host first (status 3, nothing launched): the cell ids against C, cell_dofs
// against the state's length, the facet masks against 0 .. 15, the regions against the tables, fidx against the accumulators' facets (each named once),
// the rows of ent against dst.  Every output carries SHIM_TAIL.
extern "C++" {
namespace {
int cell_list_checked(const char* who, int64_t ncell, int64_t C, int64_t nu, const int32_t* cell_dofs, const int32_t* cells) {
  if (ncell < 1 || C < 1) { g_err = std::string(who) + ": no cells"; return 3; }
  if (const int rc = indices_checked(who, cell_dofs, NLOC * C, nu)) return rc;
  return indices_checked(who, cells, ncell, C);
}
int masks_checked(const char* who, const int32_t* fmask, int64_t ncell) {
  for (int64_t i = 0; i < ncell; ++i)
    if (fmask[i] < 0 || fmask[i] > 15) { g_err = std::string(who) + ": facet mask " + std::to_string(i) + " outside 0 .. 15"; return 3; }
  return 0;
}
int regions_checked(const char* who, const int32_t* region, int64_t C) {
  for (int64_t c = 0; c < C; ++c)
    if (region[c] < 0 || region[c] >= MAX_REGIONS) { g_err = std::string(who) + ": region of cell " + std::to_string(c) + " outside the tables"; return 3; }
  return 0;
}
ElemArrays wss_arrays(Call& c, int64_t C, const double* geom, const int32_t* cell_dofs) {
  ElemArrays ea{};
  ea.geom = c.in(geom, (size_t)(10 * C));
  ea.cell_dofs = c.in(cell_dofs, (size_t)(NLOC * C));
  return ea;
}
}  // namespace
}  // extern "C++"
// U [nu]; cells, fmask [ncell]; out [12 ncell + SHIM_TAIL]: the traction coefficients [ncell][4][3]
int shim_wss(int64_t ncell, int64_t C, int64_t nu, const double* geom, const int32_t* cell_dofs, const double* U, const int32_t* cells,
             const int32_t* fmask, double mu, double* out) {
  if (const int rc = cell_list_checked("shim_wss", ncell, C, nu, cell_dofs, cells)) return rc;
  if (const int rc = masks_checked("shim_wss", fmask, ncell)) return rc;
  Call c;
  const ElemArrays ea = wss_arrays(c, C, geom, cell_dofs);
  const double* dU = c.in(U, (size_t)nu);
  const int32_t* dc = c.in(cells, (size_t)ncell);
  const int32_t* dm = c.in(fmask, (size_t)ncell);
  double* dout = c.io(out, (size_t)(12 * ncell) + SHIM_TAIL);
  SHIM_RUN(c, "launch_wss", launch_wss(c.st, ncell, ea, dU, dc, dm, mu, dout));
}
// fidx [ncell][4]: the facet (of nf) of every facet set in the mask, read there only; no facet may be named twice over the whole list
// (two lanes would then add to the same accumulators: status 3).  Accumulators in / out over 3 nf dofs:
// sum_tau, tau_prev [9 nf + SHIM_TAIL], sum_mag, sum_twssg [3 nf + SHIM_TAIL]; wss_out [9 nf + SHIM_TAIL] or null.
int shim_hemo_sample(int64_t ncell, int64_t C, int64_t nu, const double* geom, const int32_t* cell_dofs, const double* U,
                     const int32_t* cells, const int32_t* fmask, const int32_t* fidx, int64_t nf, double mu, double dt, const double* tw,
                     const double* tl, double* sum_tau, double* tau_prev, double* sum_mag, double* sum_twssg, double* wss_out) {
  if (const int rc = cell_list_checked("shim_hemo_sample", ncell, C, nu, cell_dofs, cells)) return rc;
  if (const int rc = masks_checked("shim_hemo_sample", fmask, ncell)) return rc;
  std::vector<char> named((size_t)(nf > 0 ? nf : 0), 0);
  for (int64_t i = 0; i < ncell; ++i)
    for (int f = 0; f < 4; ++f) {
      if (!(fmask[i] >> f & 1)) continue;
      const int32_t k = fidx[4 * i + f];
      if (k < 0 || k >= nf || named[(size_t)k]) {
        g_err = "shim_hemo_sample: facet " + std::to_string(f) + " of list entry " + std::to_string(i) +
                (k < 0 || k >= nf ? " outside the accumulators" : " names a facet of the accumulators a second time");
        return 3;
      }
      named[(size_t)k] = 1;
    }
  Call c;
  c.note(hemo_upload_tables(tw, tl));
  const ElemArrays ea = wss_arrays(c, C, geom, cell_dofs);
  const double* dU = c.in(U, (size_t)nu);
  const int32_t* dc = c.in(cells, (size_t)ncell);
  const int32_t* dm = c.in(fmask, (size_t)ncell);
  const int32_t* df = c.in(fidx, (size_t)(4 * ncell));
  HemoAcc acc;
  acc.sum_tau = c.io(sum_tau, (size_t)(9 * nf) + SHIM_TAIL);
  acc.tau_prev = c.io(tau_prev, (size_t)(9 * nf) + SHIM_TAIL);
  acc.sum_mag = c.io(sum_mag, (size_t)(3 * nf) + SHIM_TAIL);
  acc.sum_twssg = c.io(sum_twssg, (size_t)(3 * nf) + SHIM_TAIL);
  double* dw = c.io(wss_out, (size_t)(9 * nf) + SHIM_TAIL);
  SHIM_RUN(c, "launch_hemo_sample", launch_hemo_sample(c.st, ncell, ea, dU, dc, dm, df, mu, dt, acc, dw));
}
// sum_tau [3 ndof], sum_mag, sum_twssg [ndof]; out [5 ndof + SHIM_TAIL] = TAWSS, OSI, RRT, ECAP, TWSSG
int shim_hemo_finish(int64_t ndof, double samples, const double* sum_tau, const double* sum_mag, const double* sum_twssg, double* out) {
  if (ndof < 1) { g_err = "shim_hemo_finish: no dofs"; return 3; }
  Call c;
  HemoAcc acc{};
  acc.sum_tau = const_cast<double*>(c.in(sum_tau, (size_t)(3 * ndof)));
  acc.sum_mag = const_cast<double*>(c.in(sum_mag, (size_t)ndof));
  acc.sum_twssg = const_cast<double*>(c.in(sum_twssg, (size_t)ndof));
  double* dout = c.io(out, (size_t)(5 * ndof) + SHIM_TAIL);
  SHIM_RUN(c, "launch_hemo_finish", launch_hemo_finish(c.st, ndof, samples, acc, dout));
}
// ptr [ncell + 1] / ent [ptr[ncell]][2] = (row of dst, 4 * local vertex + component code); dst [nrows + SHIM_TAIL] in / out
int shim_spec_wss_sample(int64_t ncell, int64_t C, int64_t nu, const double* geom, const int32_t* cell_dofs, const double* U,
                         const int32_t* cells, const int32_t* fmask, const int32_t* ptr, const int32_t* ent, int64_t nrows, double mu,
                         double* dst) {
  if (const int rc = cell_list_checked("shim_spec_wss_sample", ncell, C, nu, cell_dofs, cells)) return rc;
  if (const int rc = masks_checked("shim_spec_wss_sample", fmask, ncell)) return rc;
  if (ptr[0] != 0 || nrows < 1) { g_err = "shim_spec_wss_sample: the entry ranges do not start at 0, or no rows"; return 3; }
  for (int64_t i = 0; i < ncell; ++i)
    if (ptr[i + 1] < ptr[i]) { g_err = "shim_spec_wss_sample: entry range " + std::to_string(i) + " decreases"; return 3; }
  for (int64_t e = 0; e < ptr[ncell]; ++e)
    if (ent[2 * e] < 0 || ent[2 * e] >= nrows || ent[2 * e + 1] < 0 || ent[2 * e + 1] > 15) {
      g_err = "shim_spec_wss_sample: entry " + std::to_string(e) + " outside dst, or no such vertex / component";
      return 3;
    }
  Call c;
  const ElemArrays ea = wss_arrays(c, C, geom, cell_dofs);
  const double* dU = c.in(U, (size_t)nu);
  const int32_t* dc = c.in(cells, (size_t)ncell);
  const int32_t* dm = c.in(fmask, (size_t)ncell);
  const int32_t* dp = c.in(ptr, (size_t)ncell + 1);
  const int32_t* de = c.in(ent, (size_t)(2 * ptr[ncell]));
  double* dd = c.io(dst, (size_t)nrows + SHIM_TAIL);
  SHIM_RUN(c, "launch_spec_wss_sample", launch_spec_wss_sample(c.st, ncell, ea, dU, dc, dm, dp, de, mu, dd));
}
extern "C++" {
namespace {
// the checks and uploads the three cell kernels of the solid tensors share; returns nonzero with nothing uploaded
int solid_cells(const char* who, Call& c, int64_t ncell, int64_t C, int64_t nu, const double* geom, const int32_t* cell_dofs,
                const int32_t* cell_region, const double* qw, const double* dN, const double* L, const double* U, const int32_t* cells,
                ElemArrays& ea, const double*& dU, const int32_t*& dc) {
  if (const int rc = cell_list_checked(who, ncell, C, nu, cell_dofs, cells)) return rc;
  if (const int rc = regions_checked(who, cell_region, C)) return rc;
  c.note(upload_post_tables(qw, dN, L));
  ea = wss_arrays(c, C, geom, cell_dofs);
  ea.cell_region = c.in(cell_region, (size_t)C);
  dU = c.in(U, (size_t)nu);
  dc = c.in(cells, (size_t)ncell);
  return 0;
}
}  // namespace
}  // extern "C++"
// out [80 ncell + SHIM_TAIL]: per listed cell TrueStress [4][9], GreenLagrangeStrain [4][9], MaxPrincipalStress [4], MaxPrincipalStrain [4]
int shim_stress_strain(int64_t ncell, int64_t C, int64_t nu, const double* geom, const int32_t* cell_dofs, const int32_t* cell_region,
                       const double* sc, const double* fluid, const double* solid, const double* qw, const double* dN, const double* L,
                       const double* U, const int32_t* cells, double* out) {
  Call c;
  ElemArrays ea{};
  const double* dU = nullptr;
  const int32_t* dc = nullptr;
  if (const int rc = solid_cells("shim_stress_strain", c, ncell, C, nu, geom, cell_dofs, cell_region, qw, dN, L, U, cells, ea, dU, dc)) return rc;
  const ElemParams ep = elem_params(sc, fluid, solid);
  double* dout = c.io(out, (size_t)(80 * ncell) + SHIM_TAIL);
  SHIM_RUN(c, "launch_stress_strain", launch_stress_strain(c.st, ncell, ea, ep, dU, dc, dout));
}
// frame [80 ncell + SHIM_TAIL] as out of shim_stress_strain; sums [8 ncell + SHIM_TAIL] in / out
int shim_stress_sample(int64_t ncell, int64_t C, int64_t nu, const double* geom, const int32_t* cell_dofs, const int32_t* cell_region,
                       const double* sc, const double* fluid, const double* solid, const double* qw, const double* dN, const double* L,
                       const double* U, const int32_t* cells, double* frame, double* sums) {
  Call c;
  ElemArrays ea{};
  const double* dU = nullptr;
  const int32_t* dc = nullptr;
  if (const int rc = solid_cells("shim_stress_sample", c, ncell, C, nu, geom, cell_dofs, cell_region, qw, dN, L, U, cells, ea, dU, dc)) return rc;
  const ElemParams ep = elem_params(sc, fluid, solid);
  double* df = c.io(frame, (size_t)(80 * ncell) + SHIM_TAIL);
  double* ds = c.io(sums, (size_t)(8 * ncell) + SHIM_TAIL);
  SHIM_RUN(c, "launch_stress_sample", launch_stress_sample(c.st, ncell, ea, ep, dU, dc, df, ds));
}
// sums [8 ncell]; out [8 ncell + SHIM_TAIL] = [2][ncell][4]
int shim_stress_average(int64_t ncell, double samples, const double* sums, double* out) {
  if (ncell < 1) { g_err = "shim_stress_average: no cells"; return 3; }
  Call c;
  const double* ds = c.in(sums, (size_t)(8 * ncell));
  double* dout = c.io(out, (size_t)(8 * ncell) + SHIM_TAIL);
  SHIM_RUN(c, "launch_stress_average", launch_stress_average(c.st, ncell, samples, ds, dout));
}
// dst [24 ncell + SHIM_TAIL]: rows (4 ci + a) 6 + comp of the strain (strain != 0) or the stress
int shim_tensor_sample(int64_t ncell, int64_t C, int64_t nu, int strain, const double* geom, const int32_t* cell_dofs,
                       const int32_t* cell_region, const double* sc, const double* fluid, const double* solid, const double* qw,
                       const double* dN, const double* L, const double* U, const int32_t* cells, double* dst) {
  Call c;
  ElemArrays ea{};
  const double* dU = nullptr;
  const int32_t* dc = nullptr;
  if (const int rc = solid_cells("shim_tensor_sample", c, ncell, C, nu, geom, cell_dofs, cell_region, qw, dN, L, U, cells, ea, dU, dc)) return rc;
  const ElemParams ep = elem_params(sc, fluid, solid);
  double* dd = c.io(dst, (size_t)(24 * ncell) + SHIM_TAIL);
  SHIM_RUN(c, "launch_tensor_sample", launch_tensor_sample(c.st, ncell, ea, ep, dU, dc, strain != 0, dd));
}
// amp [6 nnode] = 11, 12, 22, 23, 33, 31 per dof; mag [nnode + SHIM_TAIL]
int shim_tensor_principal(int64_t nnode, const double* amp, double* mag) {
  if (nnode < 1) { g_err = "shim_tensor_principal: no dofs"; return 3; }
  Call c;
  const double* da = c.in(amp, (size_t)(6 * nnode));
  double* dm = c.io(mag, (size_t)nnode + SHIM_TAIL);
  SHIM_RUN(c, "launch_tensor_principal", launch_tensor_principal(c.st, nnode, da, dm));
}

// ---- a live context's preconditioner arrays (FsiCtx of fsi_context.hpp, as the library was compiled) -----------------------
// shim_ctx_info: N2, V, nS, sb_nblocks, tiled, tile_nodes, tile_max_nu, schur_tiled, schur_tile, s_tile_max_nu, sweeps_fp16,
// a32_ptail, a32_tail_src, a32_tail_nnz, op32_ok, kry_fp32, drows_ok, mg_nc, mg_cnnz, mg_ready, sbmg_nc, sbmg_nblk, sbmg_ready,
// bcr_ready, the ProductForm of the FP64 products and of those on the FP32 copy (new fields go at the end: tests/kernel_shim.py
// reads them by position)
int shim_ctx_info(const FsiCtx* ctx, int64_t* out, int nout) {
  const int64_t v[] = {ctx->N2, ctx->V, ctx->nS, ctx->sb_nblocks, ctx->tiled, ctx->tile_nodes, ctx->tile_max_nu,
                       ctx->schur_tiled, ctx->schur_tile, ctx->s_tile_max_nu, ctx->sweeps_fp16,
                       ctx->prod.tail.ptail, ctx->prod.tail.src, ctx->prod.tail.nnz, ctx->prod.copy_ok, ctx->kry_fp32, ctx->prod.pairs(),
                       ctx->mg_nc, ctx->mg_cnnz, ctx->mg_ready, ctx->sbmg_nc, ctx->sbmg_nblk, ctx->sbmg_ready, fsi::host::bcr_ready(ctx),
                       ctx->prod.form.f64, ctx->prod.form.f32};
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < nout && i < k; ++i) out[i] = v[i];
  return k;
}
// What precondition_block (fsi_precond.hip) branches on and the sweep counts it takes, by position (new fields go at the end:
// tests/block_apply.py reads them by position).  iout: two_chains, drop_last_sweep, experiment, vel_jacobi, dd_early, solid_fp32,
// solid_block_jacobi, solid_fused, sweeps_fp32, sweeps_fp16, fused_sweeps, tiled, schur_fp32, schur_tiled, cheb4, cheb_its_s,
// cheb_its_f, cheb_its_p, cheb_its_d, sbmg_pre, sbmg_post, sbmg_cits, mg_pre, mg_post, mg_cits, xs_zeroed (0 / 1: the solid
// predictor's vector is known to be zero off the solid nodes), have s_vals32, s_rec, sb_rec, sb_rec32, vv_rec32 (0 / 1 each),
// debug_prec_apply.  dout: sbmg_alpha, mg_alpha, sbmg_ckappa, mg_ckappa, bcr_shift.  Returns the number of iout fields.
int shim_ctx_apply_info(const FsiCtx* ctx, int64_t* iout, int ni, double* dout, int nd) {
  const int64_t v[] = {fsi::host::block_two_chains(ctx), (ctx->tune.experiment & 4) == 0, ctx->tune.experiment, ctx->vel_jacobi,
                       ctx->dd_early, ctx->solid_fp32, ctx->solid_block_jacobi, ctx->solid_fused, ctx->sweeps_fp32, ctx->sweeps_fp16,
                       ctx->fused_sweeps, ctx->tiled, ctx->schur_fp32, ctx->schur_tiled, ctx->cheb4, ctx->cheb_its_s, ctx->cheb_its_f,
                       ctx->cheb_its_p, ctx->cheb_its_d, ctx->sbmg_pre, ctx->sbmg_post, ctx->sbmg_cits, ctx->mg_pre, ctx->mg_post,
                       ctx->mg_cits, ctx->xs_zeroed != nullptr, ctx->s_vals32.p != nullptr, ctx->s_rec.p != nullptr,
                       ctx->sb_rec.p != nullptr, ctx->sb_rec32.p != nullptr, ctx->vv_rec32.p != nullptr, ctx->debug_prec_apply};
  const double w[] = {ctx->sbmg_alpha, ctx->mg_alpha, ctx->sbmg_ckappa, ctx->mg_ckappa, ctx->tune.bcr_shift};
  const int k = (int)(sizeof(v) / sizeof(v[0])), kd = (int)(sizeof(w) / sizeof(w[0]));
  for (int i = 0; i < ni && i < k; ++i) iout[i] = v[i];
  for (int i = 0; i < nd && i < kd; ++i) dout[i] = w[i];
  return k;
}
// the factor of the solid columns' displacement entries folded into the velocity block (Avv~ = Avv + ktheta Avd, k_extract_blocks)
double shim_ctx_ktheta(const FsiCtx* ctx) { return ctx->scheme.k * ctx->scheme.th0; }
// the coarse levels' eigenvalue bounds: 0 mg_gersh, 1 sbmg_gersh (the row-sum bounds of the last rebuild), 2 mg_clmax, 3 sbmg_clmax
// (what the Chebyshev intervals use); 4 .. 7 lmax_s, lmax_f, lmax_p, lmax_d (the fine blocks' intervals end there), 8 .. 11
// cheb_kappa_s, _f, _p, _d, 12 .. 16 the flags dd_is_db, adv_is_db, dd_is_scalar, adv_solid_only, pv32_ok as 0 / 1; NaN for any
// other index
double shim_ctx_coarse(const FsiCtx* ctx, int which) {
  switch (which) {
    case 0: return ctx->mg_gersh;
    case 1: return ctx->sbmg_gersh;
    case 2: return ctx->mg_clmax;
    case 3: return ctx->sbmg_clmax;
    case 4: return ctx->lmax_s;
    case 5: return ctx->lmax_f;
    case 6: return ctx->lmax_p;
    case 7: return ctx->lmax_d;
    case 8: return ctx->cheb_kappa_s;
    case 9: return ctx->cheb_kappa_f;
    case 10: return ctx->cheb_kappa_p;
    case 11: return ctx->cheb_kappa_d;
    case 12: return ctx->dd_is_db;
    case 13: return ctx->adv_is_db;
    case 14: return ctx->dd_is_scalar;
    case 15: return ctx->adv_solid_only;
    case 16: return ctx->pv32_ok;
    default: return std::nan("");
  }
}
// Copies the named device array into host (when host is not null); *count / *elem: its length and element size.
// Status 2: no such name.
int shim_ctx_array(const FsiCtx* ctx, const char* name, void* host, int64_t* count, int* elem) {
  struct Entry { const char* name; const void* p; size_t n, sz; };
#define E(f) Entry{#f, ctx->f.p, ctx->f.n, sizeof(*ctx->f.p)}
#define EP(name, f) Entry{name, ctx->prod.f.p, ctx->prod.f.n, sizeof(*ctx->prod.f.p)}      // the monolithic operator's (MonoProduct)
  const Entry table[] = {E(nadj_ptr), E(nadj),        E(dd_chat), E(dd_rowflag), E(dd_rec),      E(tile_ploc),   E(tile_uptr),
                         E(tile_ulist), E(vv_db32),   E(vv_rec),  E(sb_ptr),     E(sb_col),      E(sb_vals),     E(sb_rec),
                         E(sb_binv12),  E(s_rowptr),  E(s_cols),  E(s_diagpos),  E(s_vals),      E(s_vals32),    E(s_rec),
                         E(s_ploc),     E(s_tile_uptr), E(s_tile_ulist), E(s_dinv), E(dd_db),    E(rowscale),    E(snode),
                         E(solver2user), E(node_solid), E(rowptr),    E(cols),        E(diagpos),     E(A),           E(vrank),
                         E(padj_ptr),   E(padj),      EP("A32", A32), EP("a32_ptr", a32_ptr), EP("a32_cols", a32_cols), EP("Ad64", Ad64), EP("Ad32", Ad32),
                         EP("drows_dd", Add), EP("drows_dv", Adv3), EP("drows_off", doff), EP("drows_cdeg", cdeg),
                         E(mg_par),     E(mg_pw),     E(mg_chptr), E(mg_child),  E(mg_chw),      E(mg_cptr),     E(mg_ccol),
                         E(mg_cfine),   E(mg_Ac),     E(mg_cc),   E(mg_d0),      E(mg_dcinv4),   E(mg_cflag),    E(sbmg_par),
                         E(sbmg_pw),    E(sbmg_chptr), E(sbmg_child), E(sbmg_chw), E(sbmg_cptr),  E(sbmg_ccol),   E(sbmg_cfine),
                         E(sbmg_cvals), E(sbmg_cbinv12), E(sbmg_flag), E(sbmg_cflag), E(sb_binv9), E(sb_dinv),   E(dd_dinv32),
                         E(vvf_dinv32),  E(vv_rec32),   E(sb_rec32),
                         E(rowptr3),    E(cols3),     E(diagpos3), E(rowptr_vp), E(cols_vp),     E(rowptr_pv),   E(cols_pv),
                         E(rowptr_pp),  E(cols_pp),   E(Mdd.vals), E(Mvv.vals),  E(Adv),         E(Avp),         E(Apv),
                         E(App),        E(Avp32),     E(Apv32),   E(vv_db),      E(adv_db),      E(dd_db32),     E(adv_rowmask),
                         E(vv_dinv),    E(mask_f),    E(mask_s),  E(ss_vals),    E(ss_src),      E(ss_rowptr),   E(ss_cols),
                         E(ss_diagpos), E(fs_rows),   E(fs_ptr),  E(fs_col),     E(fs_src),      E(sb_row),      E(sb_src),
                         E(sb_stride),  E(s_diagpos),  E(LU),       E(user2solver), E(blk),        E(sbmg_work),   E(mg_work),
                         E(ones32),     E(mg_cones),  E(bs)};
#undef E
#undef EP
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

// the colours of the multicolour ordering: out [3 x nmax] = (first_row, ngroups, group_rows) per level; returns their number
int shim_ctx_levels(const FsiCtx* ctx, int64_t* out, int nmax) {
  const int k = (int)ctx->levels.size();
  for (int i = 0; i < k && i < nmax; ++i) {
    out[3 * i] = ctx->levels[i].first_row;
    out[3 * i + 1] = ctx->levels[i].ngroups;
    out[3 * i + 2] = ctx->levels[i].group_rows;
  }
  return k;
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
  const int64_t op0 = ctx->prod.products32, dr0 = ctx->prod.pair_products;
  int rc = 0;
  if (c.ok()) {
    rc = fsi::host::spmv(ctx, dx, dy, working != 0);
    c.note(hipStreamSynchronize(ctx->stream));
  }
  counters[0] = ctx->prod.products32 - op0;
  counters[1] = ctx->prod.pair_products - dr0;
  if (const int e = c.finish("host::spmv")) return e;
  if (rc) g_err = "host::spmv: " + ctx->err;
  return rc;
}

// ---- the recycled GCR of a live context (fsi_krylov.hip): its store, one solve, one preconditioner application -----------------
// iout, by position (new fields go at the end: tests/kernel_shim.py reads them by position): cap, hw, made, free.size(), kry_fp32,
// kry_fp32_policy, ldq, ldz, hot_next, window_cols(), gcr_restarts, kry_fp32_failures_total, gcr_reorth_forced, gcr_arnoldi_steps,
// verdicts_skipped, gcr_stagnated, gcr_stalled, f64_suspect, ndof.  dout: f32_last_drift, gcr_escape.  born [cap], free_slots
// [cap] (the first free.size() are set), hot [GCR_WINDOW]; any of the three may be null.  Returns the number of iout fields.
int shim_ctx_krylov_info(const FsiCtx* ctx, int64_t* iout, int ni, double* dout, int nd, int64_t* born, int32_t* free_slots,
                         int32_t* hot) {
  const GcrStore& s = ctx->kry;
  const int64_t v[] = {s.cap, s.hw, s.made, (int64_t)s.free.size(), ctx->kry_fp32, ctx->kry_fp32_policy, ctx->ldq, ctx->ldz,
                       s.hot_next, s.window_cols(), ctx->gcr_restarts, ctx->kry_fp32_failures_total, ctx->gcr_reorth_forced,
                       ctx->gcr_arnoldi_steps, ctx->verdicts_skipped, ctx->gcr_stagnated, ctx->gcr_stalled, ctx->f64_suspect,
                       ctx->ndof};
  const double w[] = {ctx->f32_last_drift, ctx->gcr_escape};
  const int k = (int)(sizeof(v) / sizeof(v[0])), kd = (int)(sizeof(w) / sizeof(w[0]));
  for (int i = 0; i < ni && i < k; ++i) iout[i] = v[i];
  for (int i = 0; i < nd && i < kd; ++i) dout[i] = w[i];
  if (born) std::copy(s.born.begin(), s.born.end(), born);
  if (free_slots) std::copy(s.free.begin(), s.free.end(), free_slots);
  if (hot) std::copy(s.hot_slots.begin(), s.hot_slots.end(), hot);
  return k;
}
// Columns [0, hw) of the store, padding rows included: Q [hw][ldq] as raw bytes of *qelem (4 or 8) each, Z [hw][ldz], and the
// whole window Qh [GCR_WINDOW][ldq] (left alone where the context has none: FSI_KRYLOV_FP32=0).  Null pointers: *qelem only.
int shim_ctx_krylov_columns(const FsiCtx* ctx, void* Q, double* Z, double* Qh, int* qelem) {
  const size_t hw = (size_t)ctx->kry.hw, qb = ctx->kry_fp32 ? sizeof(float) : sizeof(double);
  *qelem = (int)qb;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && Q && hw) e = hipMemcpy(Q, ctx->KQ.p, hw * (size_t)ctx->ldq * qb, hipMemcpyDeviceToHost);
  if (e == hipSuccess && Z && hw) e = hipMemcpy(Z, ctx->KZ.p, hw * (size_t)ctx->ldz * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && Qh && ctx->KQh.p) e = hipMemcpy(Qh, ctx->KQh.p, (size_t)GCR_WINDOW * ctx->ldq * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) return 0;
  g_err = std::string("shim_ctx_krylov_columns: ") + hipGetErrorName(e);
  return 1;
}
// fsi::host::solve_gcr on the equilibrated system in solver ordering: rhs [ndof], x [ndof + SHIM_TAIL] (written whatever the
// status).  counters [1]: the monolithic products the solve launched (one per iteration and one per FP64 verdict).
// Status: 0, 1 = HIP error, else the FSI_ERR_* of solve_gcr (ctx->err in shim_last_error()).
int shim_ctx_solve_gcr(FsiCtx* ctx, const double* rhs, double* x, double rtol, int max_it, int32_t* iters, double* relres,
                       int64_t* counters) {
  Call c;
  const int64_t n = ctx->ndof;
  const double* drhs = c.in(rhs, (size_t)n);
  double* dx = c.io(x, (size_t)n + SHIM_TAIL);
  if (c.ok()) c.note(hipSetDevice(ctx->device));
  const int64_t sp0 = ctx->t_spmv.calls;
  int rc = 0, it = 0;
  double rr = 0.0;
  if (c.ok()) {
    rc = fsi::host::solve_gcr(ctx, drhs, dx, rtol, max_it, &it, &rr);
    c.note(hipStreamSynchronize(ctx->stream));
  }
  *iters = it;
  *relres = rr;
  counters[0] = ctx->t_spmv.calls - sp0;
  if (const int e = c.finish("host::solve_gcr")) return e;
  if (rc) g_err = "host::solve_gcr: " + ctx->err;
  return rc;
}
// z = M^-1 r through fsi::host::precondition (solver ordering); r [ndof], z [ndof + SHIM_TAIL]
int shim_ctx_precondition(FsiCtx* ctx, const double* r, double* z) {
  Call c;
  const int64_t n = ctx->ndof;
  const double* dr = c.in(r, (size_t)n);
  double* dz = c.io(z, (size_t)n + SHIM_TAIL);
  if (c.ok()) c.note(hipSetDevice(ctx->device));
  int rc = 0;
  if (c.ok()) {
    rc = fsi::host::precondition(ctx, dr, dz);
    c.note(hipStreamSynchronize(ctx->stream));
  }
  if (const int e = c.finish("host::precondition")) return e;
  if (rc) g_err = "host::precondition: " + ctx->err;
  return rc;
}

// ---- the x + d forms of a Chebyshev chain's consumers (the chain's last sweep is not launched, fsi_precond.hip) ---------------
// As the entry points of the same names without _xd, with the direction d laid out as x; every output carries SHIM_TAIL
// further elements that the launch must leave alone.
int shim_unpad_from_f32_xd(int64_t nn, const float* a, const float* d, double* b) {
  Call c;
  const float* da = c.in(a, (size_t)(4 * nn));
  const float* dd = c.in(d, (size_t)(4 * nn));
  double* db = c.io(b, (size_t)(3 * nn) + SHIM_TAIL);
  SHIM_RUN(c, "launch_unpad_from_f32", launch_unpad_from_f32(c.st, nn, da, db, dd));
}
int shim_merge_f32d_xd(int64_t N2, int64_t V, const float* xd4, const float* dd4, const double* zv, const double* zp, double* z) {
  Call c;
  const float* dxd = c.in(xd4, (size_t)(4 * N2));
  const float* ddd = c.in(dd4, (size_t)(4 * N2));
  const double* dzv = c.in(zv, (size_t)(3 * N2));
  const double* dzp = c.in(zp, (size_t)V);
  double* dz = c.io(z, (size_t)(6 * N2 + V) + SHIM_TAIL);
  SHIM_RUN(c, "launch_merge_f32d", launch_merge_f32d(c.st, N2, V, dxd, dzv, dzp, dz, ddd));
}
// full [nfull] in place
int shim_scatter3_f32_xd(int64_t nS, int64_t nfull, const int32_t* snode, const float* comp, const float* d4, double* full) {
  Call c;
  const int32_t* dsn = c.in(snode, (size_t)nS);
  const float* dco = c.in(comp, 4 * (size_t)nS);
  const float* dd = c.in(d4, 4 * (size_t)nS);
  double* dfu = c.io(full, (size_t)nfull + SHIM_TAIL);
  SHIM_RUN(c, "launch_scatter3_f32", launch_scatter3_f32(c.st, nS, dsn, dco, dfu, dd));
}
// par / pw [2 N2], d0 [N2], xc4 / dc4 [4 nc], e4 [4 N2]
int shim_mg_prolong_xd(int64_t N2, int64_t nc, const int32_t* par, const float* pw, const float* d0, const float* xc4,
                       const float* dc4, float* e4) {
  Call c;
  const int32_t* dpar = c.in(par, 2 * (size_t)N2);
  const float* dpw = c.in(pw, 2 * (size_t)N2);
  const float* dd0 = c.in(d0, (size_t)N2);
  const float* dxc = c.in(xc4, 4 * (size_t)nc);
  const float* ddc = c.in(dc4, 4 * (size_t)nc);
  float* de = c.io(e4, 4 * (size_t)N2 + SHIM_TAIL);
  SHIM_RUN(c, "launch_mg_prolong", launch_mg_prolong(c.st, N2, dpar, dpw, dd0, dxc, de, ddc));
}
// par / pw [2 nS], flag [nS], xc4 / dc4 [4 nc], e4 [4 nS]
int shim_sbmg_prolong_xd(int64_t nS, int64_t nc, const int32_t* par, const float* pw, const uint8_t* flag, const float* xc4,
                         const float* dc4, float* e4) {
  Call c;
  const int32_t* dpar = c.in(par, 2 * (size_t)nS);
  const float* dpw = c.in(pw, 2 * (size_t)nS);
  const uint8_t* dfl = c.in(flag, (size_t)nS);
  const float* dxc = c.in(xc4, 4 * (size_t)nc);
  const float* ddc = c.in(dc4, 4 * (size_t)nc);
  float* de = c.io(e4, 4 * (size_t)nS + SHIM_TAIL);
  SHIM_RUN(c, "launch_sbmg_prolong", launch_sbmg_prolong(c.st, nS, dpar, dpw, dfl, dxc, de, nullptr, nullptr, ddc));
}

}  // extern "C"
