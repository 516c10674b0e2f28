// C-ABI of libvaspfsi.so (include/vaspfsi.h): the post-processing sessions that live on the resident state over a run -
// hemodynamic indices (fsi_hemo_*), solid stress / strain (fsi_stress_*), band-pass filtered fields (fsi_band_*) and
// spectrograms (fsi_spec_*).  The arithmetic runs in the kernels of fsi_hemo / fsi_stress / fsi_band / fsi_phase / fsi_rate / fsi_spec / fsi_spi / fsi_pod .hip; the
// last two families record into one kind of history (FsiCtx::History) through the helpers below.
#include <functional>

#include "fsi_host.hpp"
#include "fsi_phase.hpp"
#include "fsi_pod.hpp"
#include "fsi_rate.hpp"
#include "fsi_room.hpp"
#include "fsi_spec.hpp"
#include "fsi_spi.hpp"
#include "fsi_vortex.hpp"

using namespace fsi;
using namespace fsi::host;

namespace {

HemoAcc hemo_acc(FsiCtx* ctx) {
  double* a = ctx->hemo.acc.p;
  const int64_t nd = 3 * ctx->hemo.nf;
  return HemoAcc{a, a + 3 * nd, a + 6 * nd, a + 7 * nd};
}

// the refusal of entry point fn: ctx->err = "<fn>: <why>" and FSI_ERR_INVALID, or null for the helpers that return a pointer
struct Refusal {
  FsiCtx* ctx;
  const char* fn;
  int operator()(const std::string& why) const { ctx->err = std::string(fn) + ": " + why; return FSI_ERR_INVALID; }
  std::nullptr_t null(const std::string& why) const { (*this)(why); return nullptr; }
};

// ---- the recorded history of a band-pass or a spectrogram session (FsiCtx::History) ---------------------------------------

// the open session of quantity q (0 d, 1 v, 2 p; among four also 3 wss; among five 3 strain, 4 stress) among all[N], or null
// with ctx->err set
template <int N> const char* quantity_range();
template <> const char* quantity_range<3>() { return ": quantity must be 0 (d), 1 (v) or 2 (p)"; }
template <> const char* quantity_range<4>() { return ": quantity must be 0 (d), 1 (v), 2 (p) or 3 (wss)"; }
template <> const char* quantity_range<5>() { return ": quantity must be 0 (d), 1 (v), 2 (p), 3 (strain) or 4 (stress)"; }
template <class S, int N>
S* open_session(FsiCtx* ctx, S (&all)[N], int32_t q, const char* fn, const char* kind, const char* begin) {
  if (q < 0 || q >= N) { ctx->err = std::string(fn) + quantity_range<N>(); return nullptr; }
  if (!all[q].open) { ctx->err = std::string(fn) + ": no " + kind + " session for this quantity (" + begin + " first)"; return nullptr; }
  return &all[q];
}
bool tensor_quantity(int32_t q) { return q == FSI_BAND_STRAIN || q == FSI_BAND_STRESS; }
FsiCtx::Band* band_session(FsiCtx* ctx, int32_t q, const char* fn) {
  return open_session(ctx, ctx->band, q, fn, "band-pass", tensor_quantity(q) ? "fsi_band_begin_cells" : "fsi_band_begin");
}
FsiCtx::Spec* spec_session(FsiCtx* ctx, int32_t q, const char* fn) {
  return open_session(ctx, ctx->spec, q, fn, "spectrogram", q == FSI_SPEC_WSS ? "fsi_spec_begin_wss" : "fsi_spec_begin");
}
// the export and import calls refuse a partitioned context before anything else, as the begin calls do
bool partitioned(FsiCtx* ctx, const char* fn) {
  if (ctx->part) ctx->err = std::string(fn) + ": partitioned contexts are not supported";
  return ctx->part;
}
// The prologue of a band-pass entry point: the open session of `quantity`, or null - with ctx->err set, unless ctx itself is
// null.  The checks an entry point asks for come in this order, which is part of its interface: the context, WHOLE_CONTEXT
// (a partitioned context is refused), VECTOR_ONLY (the quantity is d or v; vector_note: what the entry point adds to that
// refusal), the session.  A refusal of a strain / stress session is worded by its entry point and stays there.
enum BandEntry : unsigned { ANY_CONTEXT = 0, WHOLE_CONTEXT = 1, VECTOR_ONLY = 2 };
FsiCtx::Band* band_entry(FsiCtx* ctx, const char* fn, int32_t quantity, unsigned what, const char* vector_note = "") {
  if (!ctx || ((what & WHOLE_CONTEXT) && partitioned(ctx, fn))) return nullptr;
  if ((what & VECTOR_ONLY) && quantity != 0 && quantity != 1) return Refusal{ctx, fn}.null(std::string("quantity must be 0 (d) or 1 (v)") + vector_note);
  return band_session(ctx, quantity, fn);
}
// frames of the band-pass session's view of its history (fsi_band_select): those the filtered series and the amplitude have
int64_t band_frames(const FsiCtx::Band* s) { return s->sel_count < 0 ? s->frames : s->sel_count; }

// The argument checks of a begin call and the solver indices of the entries it samples at n listed nodes: i0 / i1, i1 < 0
// where an entry is one node's value and not the mean of two.  *mode (FSI_SPEC_*): one component of every node or, from
// FSI_SPEC_ALL on, the three; the pressure has one and makes *mode FSI_SPEC_X.  Entry (node i, component c of nc) sits at
// i * nc + c (node_major, the band-pass rows) or at c * n + i (the spectrogram's).  With comps (fsi_spec_begin_rows; *mode
// FSI_SPEC_X) entry i is component comps[i] of nodes[i]: a list of rows, not of nodes.
int row_lists(FsiCtx* ctx, const char* fn, int32_t quantity, int64_t n, const int32_t* nodes, const int32_t* nodes_b, int64_t capacity,
              int* mode, bool node_major, std::vector<int32_t>& i0, std::vector<int32_t>& i1, const int32_t* comps = nullptr) {
  const Refusal refuse{ctx, fn};
  if (quantity < 0 || quantity > 2) return refuse("quantity must be 0 (d), 1 (v) or 2 (p)");
  if (n <= 0 || !nodes || capacity <= 0) return refuse("needs n > 0 nodes and a capacity > 0 frames");
  if (*mode < FSI_SPEC_X || *mode > FSI_SPEC_MAG) return refuse("ncomp_mode must be FSI_SPEC_X .. FSI_SPEC_MAG");
  if (ctx->part) return refuse("partitioned contexts are not supported");
  if (n > 2 * ctx->ndof) return refuse("more nodes than the problem has dofs");
  const bool scalar = quantity == 2;
  if (scalar) *mode = FSI_SPEC_X;
  const int ncomp = scalar ? 1 : 3, nc = *mode >= FSI_SPEC_ALL ? 3 : 1;      // components a node has, and those sampled
  const int64_t limit = scalar ? ctx->V : ctx->N2, off = scalar ? 6 * ctx->N2 : 3 * ctx->N2 * quantity;
  i0.assign((size_t)(nc * n), 0);
  i1.assign((size_t)(nc * n), -1);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t a = nodes[i], b = nodes_b ? nodes_b[i] : -1;
    if (a < 0 || a >= limit || b >= limit) return refuse("node out of range");
    if (comps && !scalar && (comps[i] < 0 || comps[i] > 2)) return refuse("component out of range, needs 0 (x), 1 (y) or 2 (z)");
    for (int c = 0; c < nc; ++c) {
      const int comp = nc == 3 ? c : comps && !scalar ? comps[i] : *mode;
      const int64_t e = node_major ? i * nc + c : c * n + i;
      i0[e] = ctx->h_user2solver[off + (int64_t)ncomp * a + comp];
      if (b >= 0) i1[e] = ctx->h_user2solver[off + (int64_t)ncomp * b + comp];
    }
  }
  return FSI_OK;
}

// The room rule, once.  What the device has free, and the 1/16 of the device the context keeps for what it allocates later (a
// refreshed preconditioner, staging buffers): a session, a transform or a further buffer of one that does not fit beside it
// is refused - nothing is paged or cut.
struct Room {
  size_t free_b = 0;
  double reserve = 0.0;
  double available(double back = 0.0) const { return (double)free_b + back - reserve; }      // back: bytes the call gives back first
};
int device_room(FsiCtx* ctx, Room* r) {
  size_t total_b = 0;
  HIPCHK(hipMemGetInfo(&r->free_b, &total_b));
  r->reserve = (double)total_b / 16.0;
  return FSI_OK;
}
// `need` bytes of entry point fn, once the stream has drained: FSI_OK, or the refusal with ctx->err set (fsi_room.hpp: subject,
// layout).  back: the bytes of buffers the call releases before it allocates; what it replaces only afterwards counts as taken.
int room_for(FsiCtx* ctx, const char* fn, const char* subject, double need, const std::string& layout, double back = 0.0) {
  HIPCHK(hipStreamSynchronize(ctx->stream));
  Room room;
  FSICHK(device_room(ctx, &room));
  if (need > room.available(back)) {
    ctx->err = room_refusal(fn, subject, need, layout, room.free_b, room.reserve);
    return FSI_ERR_INVALID;
  }
  return FSI_OK;
}
std::string counted(int64_t a, const char* of_a, int64_t b, const char* of_b) {      // "<a><of_a><b><of_b>": the layouts are mostly two counts
  return std::to_string(a) + of_a + std::to_string(b) + of_b;
}

// A buffer a session wants at `count` elements: it stands if it has them (grow: or more), and is allocated otherwise.  given_back:
// what it holds now is free again before the allocation; false: it counts as taken (the buffers that go with a cell list)
struct Want {
  std::function<hipError_t()> alloc;
  double need, held;
  bool stands;
  template <class T>
  Want(DevBuf<T>* b, size_t count, bool grow = false, bool given_back = true)
      : alloc([=] { return b->alloc(count); }), need((double)(count * sizeof(T))), held(given_back ? (double)(b->n * sizeof(T)) : 0.0),
        stands(grow ? b->n >= count : b->n == count) {}
};
// The room rule for the buffers a session allocates at first use: those of `wants` that stand are kept, the rest pass one room
// check together (subject, layout: its refusal) and are allocated, their fills done when the call returns.  replace: none is kept,
// and once the call is known to fit release() gives back what they hold first.  A hipMalloc that fails behind the room check:
// release() puts the group back to nothing, and the call is refused.
template <size_t N, class Release>
int room_for(FsiCtx* ctx, const char* fn, const char* subject, const std::string& layout, const Want (&wants)[N], Release release, bool replace = false) {
  double need = 0.0, back = 0.0;
  for (const Want& w : wants)
    if (replace || !w.stands) { need += w.need; back += w.held; }
  if (need == 0.0) return FSI_OK;
  FSICHK(room_for(ctx, fn, subject, need, layout, back));
  if (replace) release();
  for (const Want& w : wants)
    if (replace || !w.stands) {
      const hipError_t e = w.alloc();
      if (e != hipSuccess) {
        (void)hipGetLastError();
        release();
        return Refusal{ctx, fn}(std::string("hipMalloc: ") + hipGetErrorString(e));
      }
    }
  HIPCHK(hipDeviceSynchronize());                                  // the allocations' own fills are done
  return FSI_OK;
}
// a further buffer of the cell list, at its first use
int cell_buffer(FsiCtx* ctx, const char* fn, const char* subject, DevBuf<double>* buf, size_t count, const std::string& layout) {
  const Want wants[] = {{buf, count, false, false}};
  return room_for(ctx, fn, subject, layout, wants, [&] { buf->release(); });
}

// What a band-pass session of `rows` rows and `capacity` frames takes (fsi_band_room, the begin calls): the history, the
// filtered series (capacity + 2 BAND_MAX_PADLEN frames), one frame each of running sums, amplitudes and magnitudes (a frame of
// magnitudes counted as a frame of rows) and the row lists.
double band_need(int64_t rows, int64_t capacity) { return 8.0 * (double)rows * (2.0 * (double)capacity + 2.0 * BAND_MAX_PADLEN + 4.0); }

// Opens a session whose begin call has passed its checks and released what the quantity had: hist[capacity][nrow],
// work[capacity + 2 BAND_MAX_PADLEN][nrow], the row lists and, where the row is the magnitude of three sampled entries, tmp.
int history_open(FsiCtx* ctx, FsiCtx::History& s, int64_t n, int64_t nrow, int64_t capacity, const std::vector<int32_t>& i0,
                 const std::vector<int32_t>& i1, bool magnitude) {
  const size_t nsamp = i0.size();
  s.nnode = n; s.nrow = nrow; s.nsamp = (int64_t)nsamp; s.capacity = capacity;
  HIPCHK(s.idx0.alloc(nsamp));
  HIPCHK(s.idx1.alloc(nsamp));
  HIPCHK(s.hist.alloc((size_t)nrow * (size_t)capacity));
  HIPCHK(s.work.alloc((size_t)nrow * (size_t)(capacity + 2 * BAND_MAX_PADLEN)));
  if (magnitude) HIPCHK(s.tmp.alloc(nsamp));
  HIPCHK(hipDeviceSynchronize());                                  // the allocations' own fills are done
  HIPCHK(hipMemcpyAsync(s.idx0.p, i0.data(), nsamp * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(s.idx1.p, i1.data(), nsamp * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s.open = true;
  return FSI_OK;
}

// What the two band-pass begin calls do once their lists stand: the room check (fsi_band_room), then the session of nnode
// nodes of ncomp components each
int band_open(FsiCtx* ctx, const char* fn, int32_t quantity, int64_t nnode, int ncomp, int64_t capacity, const std::vector<int32_t>& i0,
              const std::vector<int32_t>& i1) {
  const int64_t nrow = nnode * ncomp;
  HIPCHK(hipSetDevice(ctx->device));
  FSICHK(room_for(ctx, fn, "the session needs", band_need(nrow, capacity), counted(nrow, " rows x ", capacity, " frames, raw and filtered")));
  auto& s = ctx->band[quantity];
  s.release();                  // only now: a refused begin leaves an open session of the quantity as it was
  s.ncomp = ncomp;
  HIPCHK(s.acc.alloc((size_t)nrow));
  HIPCHK(s.amp.alloc((size_t)nrow));
  HIPCHK(s.mag.alloc((size_t)nnode));
  HIPCHK(s.part_val.alloc(BAND_ARGMAX_BLOCKS + 1));
  HIPCHK(s.part_idx.alloc(BAND_ARGMAX_BLOCKS + 1));
  return history_open(ctx, s, nnode, nrow, capacity, i0, i1, false);
}

// The next frame of the history: sample(dst) launches what fills it from dvp_["n"]; begin: the call that declared the capacity
template <class Sample>
int history_append(FsiCtx* ctx, FsiCtx::History* s, const char* fn, const char* begin, Sample sample) {
  if (s->frames >= s->capacity) { ctx->err = std::string(fn) + ": the history is full (capacity declared at " + begin + ")"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  sample(s->hist.p + (size_t)s->frames * s->nrow);
  HIPCHK(hipGetLastError());
  s->frames += 1;
  s->filtered = false;        // a filtered series no longer covers the history
  return FSI_OK;
}
// the session's entries of dvp_["n"] (or their magnitude) into the next frame of the history
int history_sample(FsiCtx* ctx, FsiCtx::History* s, const char* fn, const char* begin) {
  return history_append(ctx, s, fn, begin, [&](double* dst) {
    launch_band_sample(ctx->stream, s->nsamp, ctx->U.p, s->idx0.p, s->idx1.p, s->tmp.p ? s->tmp.p : dst);
    if (s->tmp.p) launch_spec_magnitude(ctx->stream, s->nnode, s->tmp.p, dst);
  });
}

// The checks of a filter call on a series of `frames` frames, and its coefficients as the kernels take them; ntaps_range: the
// counts the caller's message names
int filter_coef(FsiCtx* ctx, const char* fn, const char* ntaps_range, int32_t ntaps, const double* b, const double* a, const double* zi,
                int32_t padlen, int64_t frames, BandCoef* c) {
  if (ntaps < 2 || ntaps > BAND_MAX_TAPS || !b || !a || !zi || padlen < 0 || padlen > BAND_MAX_PADLEN) {
    ctx->err = std::string(fn) + ": needs " + ntaps_range + " coefficients b, a, their zi and 0 <= padlen <= 33";
    return FSI_ERR_INVALID;
  }
  if (a[0] != 1.0) { ctx->err = std::string(fn) + ": a[0] must be 1 (normalised coefficients, as scipy.signal.butter returns them)"; return FSI_ERR_INVALID; }
  if (frames <= padlen) {      // scipy: "The length of the input vector x must be greater than padlen"
    ctx->err = std::string(fn) + ": " + std::to_string(frames) + " recorded frames, the filter needs more than padlen = " + std::to_string(padlen);
    return FSI_ERR_INVALID;
  }
  *c = BandCoef{};
  for (int k = 0; k < ntaps; ++k) { c->b[k] = b[k]; c->a[k] = a[k]; }
  for (int k = 0; k < ntaps - 1; ++k) c->zi[k] = zi[k];
  return FSI_OK;
}

// Frames of nrow doubles each on the device: frame k starts at x + k * frame_stride (in doubles; a launch that takes its stride
// in frames gets frame_stride / nrow)
struct SeriesView {
  const double* x;
  int64_t frames, frame_stride;
};

// scipy.signal.filtfilt of every row into work, over the frames of the raw history that v holds
int history_filter(FsiCtx* ctx, FsiCtx::History* s, const char* fn, const char* ntaps_range, int32_t ntaps, const double* b,
                   const double* a, const double* zi, int32_t padlen, const SeriesView& v) {
  BandCoef c;
  FSICHK(filter_coef(ctx, fn, ntaps_range, ntaps, b, a, zi, padlen, v.frames, &c));
  HIPCHK(hipSetDevice(ctx->device));
  launch_band_filter(ctx->stream, s->nrow, v.frames, padlen, c, v.x, v.frame_stride / s->nrow, s->work.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s->padlen = padlen;
  s->filtered = true;
  return FSI_OK;
}

// frame k of the raw history, or of the filtered series without its guard frames
const double* history_frame(const FsiCtx::History* s, bool filtered, int64_t k) {
  return (filtered ? s->work.p + (size_t)s->padlen * s->nrow : s->hist.p) + (size_t)k * s->nrow;
}

// Where a series of a band-pass session lies, and nowhere else.  The raw frames of session g at the selection of session s (g = s:
// its own selected frames; g the session of d: the geometry that goes with them)
SeriesView raw_view(const FsiCtx::Band* g, const FsiCtx::Band* s) {
  return SeriesView{g->hist.p + (size_t)s->sel_first * g->nrow, band_frames(s), s->sel_stride * g->nrow};
}
// the series `series` (FSI_RATE_*) of s: the selected raw frames, the filtered series or fluctuation without its guard frames, the
// period's mean frames.  That the series stands is the caller's check, under its own name.
SeriesView series_view(const FsiCtx::Band* s, int32_t series) {
  if (series == FSI_RATE_RAW) return raw_view(s, s);
  if (series == FSI_RATE_SERIES) return SeriesView{history_frame(s, true, 0), band_frames(s), s->nrow};
  return SeriesView{s->phase.mean.p, s->phase.period, s->nrow};
}
// frames first, first + step, ... of a view
SeriesView taken(const SeriesView& v, int64_t first, int64_t step, int64_t count) { return SeriesView{v.x + first * v.frame_stride, count, step * v.frame_stride}; }

// The frames of a series of a cell session, for fsi_band_cell_rate, fsi_band_cell_rate_current, fsi_band_cell_vortex and
// fsi_band_cell_vortex_current, in two steps with the entry point's own checks between them.  First the session of `quantity` with a
// cell list and the series `series` (FSI_RATE_*) in place, or null with ctx->err set (ctx null: nothing to set it on).
FsiCtx::Band* cell_series_session(FsiCtx* ctx, const char* fn, int32_t quantity, int32_t series) {
  auto* s = band_entry(ctx, fn, quantity, WHOLE_CONTEXT | VECTOR_ONLY);
  if (!s) return nullptr;
  const Refusal refuse{ctx, fn};
  if (series < FSI_RATE_RAW || series > FSI_RATE_PHASE_MEAN) return refuse.null("series must be FSI_RATE_RAW, FSI_RATE_SERIES or FSI_RATE_PHASE_MEAN");
  if (s->cells.n < 1) return refuse.null("no cell list (fsi_band_cells first)");
  if (series == FSI_RATE_SERIES && !s->filtered) return refuse.null("no filtered series (fsi_band_filter or fsi_band_phase first)");
  if (series == FSI_RATE_PHASE_MEAN && (s->phase.period < 1 || !s->filtered)) return refuse.null("no phase average (fsi_band_phase first)");
  return s;
}
// Then *x: frames first, first + step, ... (`count` of them) of that series, which must hold them all
int cell_series_frames(FsiCtx* ctx, const char* fn, const FsiCtx::Band* s, int32_t series, int64_t first, int64_t step, int64_t count, SeriesView* x) {
  const Refusal refuse{ctx, fn};
  const SeriesView v = series_view(s, series);
  if (step < 1 || count < 1) return refuse("needs step >= 1 and count >= 1, got step = " + std::to_string(step) + ", count = " + std::to_string(count));
  if (first < 0 || first >= v.frames || count - 1 > (v.frames - 1 - first) / step)
    return refuse("frames " + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(step) + ", ... (" + std::to_string(count) +
                  " of them) fall outside the series of " + std::to_string(v.frames) + " frames");
  *x = taken(v, first, step, count);
  return FSI_OK;
}

// The geometry of the current configuration x = X + d, for fsi_band_cell_rate_current and fsi_band_cell_vortex_current: the
// session of d, which must be on the same nodes and hold the same recorded frames as the session s of the quantity, and for the
// phase mean a phase average of the same period over the same selection - or the refusal, under the entry point's name.  *geo:
// the d frames that go with the `count` taken frames of the series: the raw history of d at the quantity's selection, also under
// its filtered series, or d's phase means.
int cell_geometry_frames(FsiCtx* ctx, const char* fn, const FsiCtx::Band* s, int32_t series, int64_t first, int64_t step, int64_t count,
                         SeriesView* geo) {
  const Refusal refuse{ctx, fn};
  const FsiCtx::Band* g = &ctx->band[0];
  if (!g->open) return refuse("no session of quantity 0 (d): the current configuration is x = X + d (fsi_band_begin of d first)");
  if (g->h_nodes != s->h_nodes) return refuse("the session of d lists other nodes than the session of the quantity: both must be opened on the same node list");
  if (g->frames != s->frames)
    return refuse("the session of d has recorded " + std::to_string(g->frames) + " frames, the session of the quantity " + std::to_string(s->frames) +
                  ": both must hold the same frames");
  if (series == FSI_RATE_PHASE_MEAN) {
    if (g->phase.period < 1 || !g->filtered) return refuse("the session of d has no phase average (fsi_band_phase of d first)");
    if (g->phase.period != s->phase.period)
      return refuse("the phase average of d has a period of " + std::to_string(g->phase.period) + " frames, that of the quantity " +
                    std::to_string(s->phase.period));
    if (g->sel_first != s->sel_first || g->sel_stride != s->sel_stride || band_frames(g) != band_frames(s))
      return refuse("the phase average of d is over another selection of frames than that of the quantity (fsi_band_select and fsi_band_phase of d "
                    "as of the quantity)");
  }
  *geo = taken(series == FSI_RATE_PHASE_MEAN ? series_view(g, series) : raw_view(g, s), first, step, count);
  return FSI_OK;
}

// fsi_band_cell_vortex and, current, fsi_band_cell_vortex_current: per cell the nf means over the taken frames of the series -
// current: on the geometry of the d frames that go with them, and behind the means their nf numerator means - and the
// weighted sums over the cells of the means (current: of the numerators)
int cell_vortex(FsiCtx* ctx, const char* fn, bool current, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count,
                double* cells_out, double* sums_out) {
  auto* s = cell_series_session(ctx, fn, quantity, series);
  if (!s) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, fn};
  if (!cells_out && !sums_out) return refuse("cells_out and sums_out are both NULL");
  if (sums_out && !s->cells.weighted) return refuse("sums_out without weights (fsi_band_cell_weights first)");
  SeriesView x{}, geo{};
  FSICHK(cell_series_frames(ctx, fn, s, series, first, step, count, &x));
  if (current) FSICHK(cell_geometry_frames(ctx, fn, s, series, first, step, count, &geo));
  HIPCHK(hipSetDevice(ctx->device));
  auto& c = s->cells;
  const int nf = current ? FSI_VORTEX_CURRENT_FIELDS : FSI_VORTEX_FIELDS;
  const size_t n = (size_t)c.n, nblock = (size_t)cell_wsum_blocks(c.n), rows = current ? 2 * nf : nf;
  DevBuf<double>&out = c.vortex[current].out, &part = c.vortex[current].part;
  FSICHK(cell_buffer(ctx, fn, current ? "the twelve results need" : "the five results need", &out, rows * n, counted(c.n, " cells x ", 8 * rows, "")));
  if (sums_out)
    FSICHK(cell_buffer(ctx, fn, "the partial sums need", &part, nf * (nblock + 1), counted(nblock, " groups of 256 cells and the sums x ", 8 * nf, "")));
  if (current) launch_cell_vortex_current(ctx->stream, c.n, c.conn.p, c.gl.p, x.x, x.frame_stride, geo.x, geo.frame_stride, count, out.p);
  else launch_cell_vortex(ctx->stream, c.n, c.conn.p, c.gl.p, x.x, x.frame_stride, count, out.p);
  HIPCHK(hipGetLastError());
  if (cells_out) HIPCHK(hipMemcpyAsync(cells_out, out.p, nf * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (sums_out) {      // current: the bulk sums are those of the numerators, rows 6 .. 11
    double* sums = part.p + nf * nblock;
    launch_cell_wsum(ctx->stream, c.n, nf, c.weight.p, out.p + (rows - nf) * n, part.p, sums);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums_out, sums, nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

// raw frames first .. first + count - 1 of the history to the host, out[count][nrow]: frame-major, so one copy, behind
// whatever was sampled on the stream; it has finished when the call returns
int history_export(FsiCtx* ctx, const FsiCtx::History* s, const char* fn, int64_t first, int64_t count, double* out) {
  if (!out) { ctx->err = std::string(fn) + ": out is NULL"; return FSI_ERR_INVALID; }
  if (first < 0 || count < 1 || first > s->frames - count) {
    ctx->err = std::string(fn) + ": needs first >= 0, count >= 1 and first + count <= the " + std::to_string(s->frames) + " recorded frames";
    return FSI_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out, s->hist.p + (size_t)first * s->nrow, (size_t)count * (size_t)s->nrow * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

// count frames appended to the history from the host, frames[count][nrow], as count samples would have left them; the
// caller's array is free again when the call returns
int history_import(FsiCtx* ctx, FsiCtx::History* s, const char* fn, int64_t count, const double* frames) {
  if (count < 1 || !frames) { ctx->err = std::string(fn) + ": needs count >= 1 frames"; return FSI_ERR_INVALID; }
  if (count > s->capacity - s->frames) {
    ctx->err = std::string(fn) + ": " + std::to_string(s->frames) + " recorded frames + " + std::to_string(count) + " exceed the capacity of " +
               std::to_string(s->capacity);
    return FSI_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(s->hist.p + (size_t)s->frames * s->nrow, frames, (size_t)count * (size_t)s->nrow * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s->frames += count;
  s->filtered = false;        // a filtered series no longer covers the history
  return FSI_OK;
}

// sums of a hemodynamics or a stress / strain session to the host and back: n doubles, with the sample count
int sums_export(FsiCtx* ctx, const char* fn, const double* sums, size_t n, int64_t have, double* out, int64_t* samples) {
  if (!out) { ctx->err = std::string(fn) + ": null output"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out, sums, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (samples) *samples = have;
  return FSI_OK;
}
int sums_import(FsiCtx* ctx, const char* fn, double* sums, size_t n, const double* in, int64_t samples, int64_t* have) {
  if (!in || samples < 0) { ctx->err = std::string(fn) + ": needs the sums and samples >= 0"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(sums, in, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *have = samples;
  return FSI_OK;
}

template <class S, int N>
int end_session(FsiCtx* ctx, S (&all)[N], int32_t q, const char* fn) {
  if (q < 0 || q >= N) { ctx->err = std::string(fn) + quantity_range<N>(); return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  all[q].release();
  return FSI_OK;
}

// What a spectrogram session takes (fsi_spec_room, the begin calls): the raw and the filtered history and the sampled vector of
// the magnitude (nsamp entries, two lists), as band_need; with them what the transforms allocate at the end of the run, so that a
// history that fits here is not refused there: one pass of SPEC_BINS bins of a periodogram's tables over all frames, and the
// means of capacity / 4 segments.
double spec_need(int64_t nrow, int64_t nsamp, int64_t capacity) {
  return 8.0 * (double)nrow * (2.0 * (double)capacity + 2.0 * BAND_MAX_PADLEN) + 16.0 * (double)nsamp +
         16.0 * SPEC_BINS * (double)capacity + 8.0 * (double)nrow * ((double)capacity / 4.0 + 2.0);
}
// The room check of the three spectrogram begin calls
int spec_room_for(FsiCtx* ctx, const char* fn, int64_t nrow, int64_t nsamp, int64_t capacity) {
  HIPCHK(hipSetDevice(ctx->device));
  return room_for(ctx, fn, "the session needs", spec_need(nrow, nsamp, capacity),
                  counted(nrow, " rows x ", capacity, " frames, raw and filtered, and the transforms' tables"));
}

// What fsi_spec_begin and fsi_spec_begin_rows do once their row lists stand: the room check, then the session.
int spec_open(FsiCtx* ctx, const char* fn, int32_t quantity, int64_t n, int64_t nrow, int mode, int64_t capacity,
              const std::vector<int32_t>& i0, const std::vector<int32_t>& i1) {
  FSICHK(spec_room_for(ctx, fn, nrow, (int64_t)i0.size(), capacity));
  auto& s = ctx->spec[quantity];
  s.release();                  // only now: a refused begin leaves an open session of the quantity as it was
  s.mode = mode;
  return history_open(ctx, s, n, nrow, capacity, i0, i1, mode == FSI_SPEC_MAG);
}

// The average over the session's rows of the one-sided power of nseg segments of K frames, `step` frames apart, transformed
// at length nfft >= K: mean, then per slab of bins the host's tables, k_spec_power and k_spec_reduce.  out[(nfft / 2 + 1)][nseg].
// carried (fsi_spec_*_sum): the session holds rows first_row ... of a longer list, out is the caller's carry - the sum over the
// row blocks before first_row on entry (read only where first_row > 0), with this session's blocks added on return, divided by
// total_rows where that is > 0.  A refused or failed call leaves out untouched either way.
int spec_power(FsiCtx* ctx, FsiCtx::Spec* s, const char* fn, int64_t K, int64_t step, int64_t nseg, int64_t nfft, const double* window,
               int32_t scaling, double fs, double* out, bool carried = false, int64_t first_row = 0, int64_t total_rows = 0) {
  const int64_t nbins = nfft / 2 + 1, nblk = spec_blocks(s->nrow);
  double sw = 0.0, sw2 = 0.0;
  for (int64_t j = 0; j < K; ++j) { sw += window[j]; sw2 += window[j] * window[j]; }
  const double scale = scaling == FSI_SPEC_DENSITY ? 1.0 / (fs * sw2) : 1.0 / (sw * sw);
  if (!std::isfinite(scale) || scale <= 0.0) { ctx->err = std::string(fn) + ": the window gives no finite scale"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  // what one call holds on the device: means, window and result, and per bin of a slab two table columns and the row blocks'
  // partial sums.  The slab is as many bins as fit beside the 1/16 of the device the context keeps (at most 1 GiB of tables:
  // they are made on the host); if not even one pass of SPEC_BINS bins fits, the call is refused - nothing is paged.
  const double fixed = 8.0 * ((double)nseg * (double)s->nrow + (double)K + (double)nbins * (double)nseg);
  const double per_bin = 8.0 * (2.0 * (double)K + (double)nseg * (double)nblk);
  const int64_t min_slab = nbins < SPEC_BINS ? nbins : SPEC_BINS;
  Room room;
  FSICHK(device_room(ctx, &room));
  const double avail = (double)room.free_b - room.reserve - fixed;
  if (avail < per_bin * (double)min_slab) {
    ctx->err = room_refusal(fn, "the transform needs", fixed + per_bin * (double)min_slab,
                            "tables of " + counted(K, " frames x ", min_slab, " of ") + counted(nbins, " bins, cos and sin, ", nseg, " segments x ") +
                                std::to_string(s->nrow) + " rows of means and partial sums, and the result",
                            room.free_b, room.reserve);
    return FSI_ERR_INVALID;
  }
  // the host makes the tables: cos / sin of nfft angles and one slab's columns.  A transform length whose tables the host
  // should not be asked for is refused like one that does not fit the device, not left to std::bad_alloc
  if (nfft > SPEC_MAX_NFFT) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: nfft = %lld, the host's cos / sin tables are limited to %lld angles", fn, (long long)nfft, (long long)SPEC_MAX_NFFT);
    ctx->err = msg;
    return FSI_ERR_INVALID;
  }
  int64_t slab = nbins;
  const double cap = std::min(avail / per_bin, (double)(1ll << 30) / (16.0 * (double)K));
  if ((double)slab > cap) slab = std::max<int64_t>(min_slab, (int64_t)cap / SPEC_BINS * SPEC_BINS);
  struct Bufs {
    DevBuf<double> mean, w, Ct, St, part, res;
    ~Bufs() { mean.release(); w.release(); Ct.release(); St.release(); part.release(); res.release(); }
  } bufs;
  auto &mean = bufs.mean, &w = bufs.w, &Ct = bufs.Ct, &St = bufs.St, &part = bufs.part, &res = bufs.res;
  HIPCHK(mean.alloc((size_t)(nseg * s->nrow)));
  HIPCHK(w.alloc((size_t)K));
  HIPCHK(Ct.alloc((size_t)(K * slab)));
  HIPCHK(St.alloc((size_t)(K * slab)));
  HIPCHK(part.alloc((size_t)(nseg * nblk * slab)));
  HIPCHK(res.alloc((size_t)(nbins * nseg)));
  HIPCHK(hipDeviceSynchronize());
  int rc = FSI_OK;
  std::string why;
  auto chk = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == FSI_OK) { rc = FSI_ERR_DEVICE; why = std::string(what) + ": " + hipGetErrorString(e); } return e == hipSuccess; };
  const double* x = history_frame(s, s->filtered, 0);
  // cos / sin(2 pi m / nfft), m = 0 .. nfft - 1, once; a table entry is that of m = j k mod nfft
  std::vector<double> cosm, sinm, hc, hs;
  try {
    cosm.resize((size_t)nfft); sinm.resize((size_t)nfft); hc.resize((size_t)(K * slab)); hs.resize((size_t)(K * slab));
  } catch (const std::bad_alloc&) {
    ctx->err = std::string(fn) + ": the host has no memory for the cos / sin tables (" + std::to_string(16 * (nfft + K * slab)) + " bytes)";
    return FSI_ERR_INVALID;
  }
  const long double tau = 2.0L * 3.14159265358979323846264338327950288L;      // the angle in extended precision: an entry is the
  for (int64_t m = 0; m < nfft; ++m) {                                       // correctly rounded cos / sin to within its last bit
    const long double ang = tau * (long double)m / (long double)nfft;
    cosm[m] = (double)cosl(ang);
    sinm[m] = (double)sinl(ang);
  }
  if (carried && first_row > 0) chk(hipMemcpyAsync(res.p, out, (size_t)(nbins * nseg) * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "carry upload");
  if (rc == FSI_OK && chk(hipMemcpyAsync(w.p, window, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "window upload")) {
    launch_spec_mean(ctx->stream, s->nrow, K, step, nseg, x, mean.p);
    chk(hipGetLastError(), "k_spec_mean");
  }
  for (int64_t bin0 = 0; bin0 < nbins && rc == FSI_OK; bin0 += slab) {
    const int64_t nb = std::min(slab, nbins - bin0);
    for (int64_t j = 0; j < K; ++j)
      for (int64_t b = 0; b < nb; ++b) {
        const int64_t m = (int64_t)(((unsigned __int128)j * (unsigned __int128)(bin0 + b)) % (unsigned __int128)nfft);
        hc[j * nb + b] = cosm[m];
        hs[j * nb + b] = sinm[m];
      }
    if (!chk(hipMemcpyAsync(Ct.p, hc.data(), (size_t)(K * nb) * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "table upload")) break;
    if (!chk(hipMemcpyAsync(St.p, hs.data(), (size_t)(K * nb) * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "table upload")) break;
    launch_spec_power(ctx->stream, s->nrow, K, step, nseg, nb, bin0, nfft % 2 == 0 ? nfft / 2 : -1, scale, x, mean.p, w.p, Ct.p, St.p, part.p);
    if (carried) launch_spec_reduce_sum(ctx->stream, s->nrow, nseg, nb, bin0, first_row, total_rows, part.p, res.p);
    else launch_spec_reduce(ctx->stream, s->nrow, nseg, nb, bin0, part.p, res.p);
    if (!chk(hipGetLastError(), "k_spec_power")) break;
    if (!chk(hipStreamSynchronize(ctx->stream), "k_spec_power")) break;      // the host tables are refilled for the next slab
  }
  if (rc == FSI_OK && chk(hipMemcpyAsync(out, res.p, (size_t)(nbins * nseg) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "result"))
    chk(hipStreamSynchronize(ctx->stream), "result");
  if (rc != FSI_OK) ctx->err = std::string(fn) + ": " + why;
  return rc;
}

// The checks of fsi_spec_spectrogram(_sum) and fsi_spec_periodogram(_sum) (periodogram: nperseg, noverlap and nfft are not
// read) and the transform.  carried: out_power is the carry of a _sum call (spec_power), whose own checks come first.
int spec_transform(FsiCtx* ctx, const char* name, bool periodogram, int32_t quantity, int64_t nperseg, int64_t noverlap, int64_t nfft, const double* window,
                   int32_t scaling, double fs, double* out_power, bool carried, int64_t first_row, int64_t total_rows) {
  if (!ctx) return FSI_ERR_INVALID;
  const std::string fn(name);
  auto* s = spec_session(ctx, quantity, name);
  if (!s) return FSI_ERR_INVALID;
  if (!window || !out_power || (scaling != FSI_SPEC_SPECTRUM && scaling != FSI_SPEC_DENSITY) || !(fs > 0.0)) {
    ctx->err = fn + ": needs a window, " + (carried ? "a carry" : "an output") + ", scaling FSI_SPEC_SPECTRUM or FSI_SPEC_DENSITY and fs > 0";
    return FSI_ERR_INVALID;
  }
  if (carried) {
    if (first_row < 0 || first_row % SPEC_ROWS != 0) {
      ctx->err = fn + ": first_row = " + std::to_string(first_row) + ", a strip starts at a multiple of " + std::to_string(SPEC_ROWS) + " rows (the row blocks of the sum)";
      return FSI_ERR_INVALID;
    }
    if (total_rows == 0 && s->nrow % SPEC_ROWS != 0) {
      ctx->err = fn + ": the session has " + std::to_string(s->nrow) + " rows and is not the last strip (total_rows = 0): a later strip's row blocks would be cut "
                 "differently, needs a multiple of " + std::to_string(SPEC_ROWS);
      return FSI_ERR_INVALID;
    }
    if (total_rows != 0 && total_rows != first_row + s->nrow) {
      ctx->err = fn + ": total_rows = " + std::to_string(total_rows) + ", the last strip ends at first_row + rows = " + std::to_string(first_row) + " + " +
                 std::to_string(s->nrow);
      return FSI_ERR_INVALID;
    }
  }
  if (periodogram) {
    if (s->frames < 1) { ctx->err = fn + ": no recorded frames"; return FSI_ERR_INVALID; }
    return spec_power(ctx, s, name, s->frames, s->frames, 1, s->frames, window, scaling, fs, out_power, carried, first_row, total_rows);
  }
  if (nperseg < 1 || noverlap < 0 || noverlap >= nperseg || nfft < nperseg) {
    ctx->err = fn + ": needs nperseg >= 1, 0 <= noverlap < nperseg and nfft >= nperseg";
    return FSI_ERR_INVALID;
  }
  if (s->frames < nperseg) {
    ctx->err = fn + ": " + std::to_string(s->frames) + " recorded frames, one segment needs nperseg = " + std::to_string(nperseg);
    return FSI_ERR_INVALID;
  }
  const int64_t step = nperseg - noverlap, nseg = (s->frames - noverlap) / step;
  if (nseg > 65535) { ctx->err = fn + ": more than 65535 segments"; return FSI_ERR_INVALID; }
  return spec_power(ctx, s, name, nperseg, step, nseg, nfft, window, scaling, fs, out_power, carried, first_row, total_rows);
}

// The ranks of a selection call: 0 <= rank < n each, at most BAND_SEL_MAX_RANKS distinct ones.  uniq: those, ascending;
// where[k]: the place of ranks[k] among them (both nullable: the checks alone).
int ranks_checked(FsiCtx* ctx, const char* fn, int64_t n, int32_t nranks, const int64_t* ranks, std::vector<int64_t>* uniq, std::vector<int>* where) {
  if (nranks < 1 || !ranks) { ctx->err = std::string(fn) + ": needs nranks >= 1 ranks"; return FSI_ERR_INVALID; }
  std::vector<int64_t> u(ranks, ranks + nranks);
  for (int64_t r : u)
    if (r < 0 || r >= n) { ctx->err = std::string(fn) + ": rank " + std::to_string(r) + " out of range, needs 0 <= rank < " + std::to_string(n); return FSI_ERR_INVALID; }
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  if ((int64_t)u.size() > BAND_SEL_MAX_RANKS) {
    ctx->err = std::string(fn) + ": " + std::to_string(u.size()) + " distinct ranks, one call takes " + std::to_string(BAND_SEL_MAX_RANKS);
    return FSI_ERR_INVALID;
  }
  if (where) {
    where->resize((size_t)nranks);
    for (int32_t k = 0; k < nranks; ++k) (*where)[k] = (int)(std::lower_bound(u.begin(), u.end(), ranks[k]) - u.begin());
  }
  if (uniq) uniq->swap(u);
  return FSI_OK;
}

// values[frame][nranks], nan_counts[frame] of `frames` frames of n elements at x (device), `stride` elements apart: the
// selection kernel on the distinct ranks, copied back and spread over the ranks asked for
int order_statistics(FsiCtx* ctx, const char* fn, int64_t n, int64_t frames, int64_t stride, const double* x, int32_t nranks, const int64_t* ranks,
                     double* values, int64_t* nan_counts) {
  std::vector<int64_t> uniq;
  std::vector<int> where;
  FSICHK(ranks_checked(ctx, fn, n, nranks, ranks, &uniq, &where));
  const size_t nu = uniq.size();
  DevBuf<int64_t> d_ranks, d_nans;      // live for this call
  DevBuf<double> d_out;
  HIPCHK(d_ranks.alloc(nu));
  HIPCHK(d_nans.alloc((size_t)frames));
  HIPCHK(d_out.alloc(nu * (size_t)frames));
  HIPCHK(hipDeviceSynchronize());                                  // the allocations' own fills are done
  std::vector<double> got(nu * (size_t)frames);
  HIPCHK(hipMemcpyAsync(d_ranks.p, uniq.data(), nu * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  launch_band_select(ctx->stream, n, frames, stride, x, (int)nu, d_ranks.p, d_out.p, d_nans.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(got.data(), d_out.p, got.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(nan_counts, d_nans.p, (size_t)frames * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int64_t f = 0; f < frames; ++f)
    for (int32_t k = 0; k < nranks; ++k) values[f * nranks + k] = got[(size_t)f * nu + (size_t)where[k]];
  return FSI_OK;
}
}  // namespace

extern "C" {

int fsi_hemo_begin(FsiCtx* ctx, int64_t nf, const int32_t* facet_cells, const int32_t* facet_local, double mu,
                   double dt_sample) {
  if (!ctx) return FSI_ERR_INVALID;
  if (nf <= 0 || !facet_cells || !facet_local || !(mu > 0.0) || !(dt_sample > 0.0)) {
    ctx->err = "fsi_hemo_begin: needs nf > 0 facets, mu > 0 and dt_sample > 0";
    return FSI_ERR_INVALID;
  }
  if (ctx->part) { ctx->err = "fsi_hemo_begin: partitioned contexts are not supported"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  // as fsi_wall_shear_stress: one projection per boundary cell, a mask of its listed facets, and here the user index of each
  std::vector<int32_t> ucell, mask, fidx;
  {
    std::vector<std::pair<int32_t, int64_t>> order((size_t)nf);
    for (int64_t f = 0; f < nf; ++f) {
      if (facet_cells[f] < 0 || facet_cells[f] >= ctx->C || facet_local[f] < 0 || facet_local[f] > 3) {
        ctx->err = "fsi_hemo_begin: facet cell / local index out of range";
        return FSI_ERR_INVALID;
      }
      order[f] = {facet_cells[f], f};
    }
    std::sort(order.begin(), order.end());
    for (int64_t k = 0; k < nf; ++k) {
      const int64_t f = order[k].second;
      if (k == 0 || order[k].first != order[k - 1].first) {
        ucell.push_back(order[k].first);
        mask.push_back(0);
        for (int j = 0; j < 4; ++j) fidx.push_back(-1);
      }
      if (mask.back() & (1 << facet_local[f])) { ctx->err = "fsi_hemo_begin: a facet is listed twice"; return FSI_ERR_INVALID; }
      mask.back() |= 1 << facet_local[f];
      fidx[(ucell.size() - 1) * 4 + facet_local[f]] = (int32_t)f;
    }
  }
  // 12-point degree-6 rule on the reference triangle (FIAT _triangle_scheme(6), oracle.fsi_oracle.triangle12)
  double tw[12], tl[12][3];
  {
    const double pa[2] = {0.063089014491502, 0.249286745170910}, pw[2] = {0.050844906370207, 0.116786275726379};
    double px[12], py[12];
    int q = 0;
    for (int o = 0; o < 2; ++o) {
      const double a = pa[o], b = 1.0 - 2.0 * a;
      const double xy[3][2] = {{a, a}, {b, a}, {a, b}};
      for (int k = 0; k < 3; ++k, ++q) { px[q] = xy[k][0]; py[q] = xy[k][1]; tw[q] = pw[o] / 2.0; }
    }
    const double a = 0.053145049844817, b = 0.310352451033784, c = 1.0 - a - b;
    const double xy[6][2] = {{a, b}, {b, a}, {a, c}, {c, a}, {b, c}, {c, b}};
    for (int k = 0; k < 6; ++k, ++q) { px[q] = xy[k][0]; py[q] = xy[k][1]; tw[q] = 0.082851075618374 / 2.0; }
    for (q = 0; q < 12; ++q) { tl[q][0] = 1.0 - px[q] - py[q]; tl[q][1] = px[q]; tl[q][2] = py[q]; }
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hemo_upload_tables(tw, &tl[0][0]));
  auto& h = ctx->hemo;
  h.release();
  h.nf = nf;
  h.ncell = (int64_t)ucell.size();
  h.mu = mu;
  h.dt = dt_sample;
  HIPCHK(h.cells.alloc(ucell.size()));
  HIPCHK(h.mask.alloc(mask.size()));
  HIPCHK(h.fidx.alloc(fidx.size()));
  HIPCHK(h.acc.alloc((size_t)nf * 24));
  HIPCHK(h.out.alloc((size_t)nf * 15));
  HIPCHK(hipDeviceSynchronize());                                  // the allocations' own fills are done
  HIPCHK(hipMemcpyAsync(h.cells.p, ucell.data(), ucell.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(h.mask.p, mask.data(), mask.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(h.fidx.p, fidx.data(), fidx.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(h.acc.p, 0, h.acc.n * sizeof(double), ctx->stream));   // zero whatever FSI_DEBUG_POISON filled in
  HIPCHK(hipStreamSynchronize(ctx->stream));
  h.open = true;
  return FSI_OK;
}

int fsi_hemo_sample(FsiCtx* ctx, double* wss_out) {
  if (!ctx) return FSI_ERR_INVALID;
  auto& h = ctx->hemo;
  if (!h.open) { ctx->err = "fsi_hemo_sample: no hemodynamics session (fsi_hemo_begin first)"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  launch_hemo_sample(ctx->stream, h.ncell, elem_arrays(ctx), ctx->U.p, h.cells.p, h.mask.p, h.fidx.p, h.mu, h.dt, hemo_acc(ctx),
                     wss_out ? h.out.p : nullptr);
  HIPCHK(hipGetLastError());
  h.samples += 1;
  if (wss_out) {
    HIPCHK(hipMemcpyAsync(wss_out, h.out.p, (size_t)h.nf * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return FSI_OK;
}

int fsi_hemo_indices(FsiCtx* ctx, double* out, int64_t* samples) {
  if (!ctx) return FSI_ERR_INVALID;
  auto& h = ctx->hemo;
  if (!h.open) { ctx->err = "fsi_hemo_indices: no hemodynamics session (fsi_hemo_begin first)"; return FSI_ERR_INVALID; }
  if (h.samples == 0) { ctx->err = "fsi_hemo_indices: no sample taken yet"; return FSI_ERR_INVALID; }
  if (!out) { ctx->err = "fsi_hemo_indices: null output"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  launch_hemo_finish(ctx->stream, 3 * h.nf, (double)h.samples, hemo_acc(ctx), h.out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, h.out.p, (size_t)h.nf * 15 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (samples) *samples = h.samples;
  return FSI_OK;
}

int fsi_hemo_export(FsiCtx* ctx, double* acc_out, int64_t* samples) {
  if (!ctx) return FSI_ERR_INVALID;
  if (partitioned(ctx, "fsi_hemo_export")) return FSI_ERR_INVALID;
  auto& h = ctx->hemo;
  if (!h.open) { ctx->err = "fsi_hemo_export: no hemodynamics session (fsi_hemo_begin first)"; return FSI_ERR_INVALID; }
  return sums_export(ctx, "fsi_hemo_export", h.acc.p, (size_t)h.nf * 24, h.samples, acc_out, samples);
}

int fsi_hemo_import(FsiCtx* ctx, const double* acc, int64_t samples) {
  if (!ctx) return FSI_ERR_INVALID;
  if (partitioned(ctx, "fsi_hemo_import")) return FSI_ERR_INVALID;
  auto& h = ctx->hemo;
  if (!h.open) { ctx->err = "fsi_hemo_import: no hemodynamics session (fsi_hemo_begin first)"; return FSI_ERR_INVALID; }
  return sums_import(ctx, "fsi_hemo_import", h.acc.p, (size_t)h.nf * 24, acc, samples, &h.samples);
}

int fsi_hemo_end(FsiCtx* ctx) {
  if (!ctx) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->hemo.release();
  return FSI_OK;
}

int fsi_stress_begin(FsiCtx* ctx, int64_t n, const int32_t* cells) {
  if (!ctx) return FSI_ERR_INVALID;
  if (n <= 0 || !cells) { ctx->err = "fsi_stress_begin: needs n > 0 cells"; return FSI_ERR_INVALID; }
  if (ctx->part) { ctx->err = "fsi_stress_begin: partitioned contexts are not supported"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<int32_t> kinds((size_t)ctx->C);
  HIPCHK(hipMemcpy(kinds.data(), ctx->cell_kind.p, (size_t)ctx->C * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) {
    if (cells[i] < 0 || cells[i] >= ctx->C) { ctx->err = "fsi_stress_begin: cell out of range"; return FSI_ERR_INVALID; }
    if (kinds[cells[i]] != 1) { ctx->err = "fsi_stress_begin: cell is not a solid cell"; return FSI_ERR_INVALID; }
  }
  auto& s = ctx->stress;
  s.release();
  s.n = n;
  HIPCHK(s.cells.alloc((size_t)n));
  HIPCHK(s.frame.alloc((size_t)n * 80));
  HIPCHK(s.sums.alloc((size_t)n * 8));
  HIPCHK(s.avg.alloc((size_t)n * 8));
  HIPCHK(hipDeviceSynchronize());                                  // the allocations' own fills are done
  HIPCHK(hipMemcpyAsync(s.cells.p, cells, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(s.sums.p, 0, s.sums.n * sizeof(double), ctx->stream));  // zero whatever FSI_DEBUG_POISON filled in
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s.open = true;
  return FSI_OK;
}

int fsi_stress_sample(FsiCtx* ctx, double* frame_out) {
  if (!ctx) return FSI_ERR_INVALID;
  auto& s = ctx->stress;
  if (!s.open) { ctx->err = "fsi_stress_sample: no stress / strain session (fsi_stress_begin first)"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  launch_stress_sample(ctx->stream, s.n, elem_arrays(ctx), elem_params(ctx), ctx->U.p, s.cells.p, s.frame.p, s.sums.p);
  HIPCHK(hipGetLastError());
  s.samples += 1;
  if (frame_out) {
    HIPCHK(hipMemcpyAsync(frame_out, s.frame.p, (size_t)s.n * 80 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return FSI_OK;
}

int fsi_stress_averages(FsiCtx* ctx, double* out, int64_t* samples) {
  if (!ctx) return FSI_ERR_INVALID;
  auto& s = ctx->stress;
  if (!s.open) { ctx->err = "fsi_stress_averages: no stress / strain session (fsi_stress_begin first)"; return FSI_ERR_INVALID; }
  if (s.samples == 0) { ctx->err = "fsi_stress_averages: no sample taken yet"; return FSI_ERR_INVALID; }
  if (!out) { ctx->err = "fsi_stress_averages: null output"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  launch_stress_average(ctx->stream, s.n, (double)s.samples, s.sums.p, s.avg.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, s.avg.p, (size_t)s.n * 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (samples) *samples = s.samples;
  return FSI_OK;
}

int fsi_stress_export(FsiCtx* ctx, double* sums_out, int64_t* samples) {
  if (!ctx) return FSI_ERR_INVALID;
  if (partitioned(ctx, "fsi_stress_export")) return FSI_ERR_INVALID;
  auto& s = ctx->stress;
  if (!s.open) { ctx->err = "fsi_stress_export: no stress / strain session (fsi_stress_begin first)"; return FSI_ERR_INVALID; }
  return sums_export(ctx, "fsi_stress_export", s.sums.p, (size_t)s.n * 8, s.samples, sums_out, samples);
}

int fsi_stress_import(FsiCtx* ctx, const double* sums, int64_t samples) {
  if (!ctx) return FSI_ERR_INVALID;
  if (partitioned(ctx, "fsi_stress_import")) return FSI_ERR_INVALID;
  auto& s = ctx->stress;
  if (!s.open) { ctx->err = "fsi_stress_import: no stress / strain session (fsi_stress_begin first)"; return FSI_ERR_INVALID; }
  return sums_import(ctx, "fsi_stress_import", s.sums.p, (size_t)s.n * 8, sums, samples, &s.samples);
}

int fsi_stress_end(FsiCtx* ctx) {
  if (!ctx) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->stress.release();
  return FSI_OK;
}

int fsi_band_begin(FsiCtx* ctx, int32_t quantity, int64_t n, const int32_t* nodes, const int32_t* nodes_b, int64_t capacity) {
  if (!ctx) return FSI_ERR_INVALID;
  int mode = FSI_SPEC_ALL;      // every component of a node, node-major: a frame is the (n, ncomp) array of a Visualization file
  std::vector<int32_t> i0, i1;
  FSICHK(row_lists(ctx, "fsi_band_begin", quantity, n, nodes, nodes_b, capacity, &mode, true, i0, i1));
  FSICHK(band_open(ctx, "fsi_band_begin", quantity, n, (int)((int64_t)i0.size() / n), capacity, i0, i1));
  auto& s = ctx->band[quantity];
  s.h_nodes.assign(nodes, nodes + n);            // for fsi_band_cells: a row that is the mean of two nodes is no node's
  if (nodes_b)
    for (int64_t i = 0; i < n; ++i)
      if (nodes_b[i] >= 0) s.h_nodes[i] = -1;
  return FSI_OK;
}

int fsi_band_begin_cells(FsiCtx* ctx, int32_t quantity, int64_t n, const int32_t* cells, int64_t capacity) {
  if (!ctx) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_band_begin_cells"};
  if (!tensor_quantity(quantity)) return refuse("quantity must be 3 (strain) or 4 (stress)");
  if (n <= 0 || !cells || capacity <= 0) return refuse("needs n > 0 cells and a capacity > 0 frames");
  if (ctx->part) return refuse("partitioned contexts are not supported");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<int32_t> kinds((size_t)ctx->C);      // as fsi_stress_begin: range and kind on the host, before anything is uploaded
  HIPCHK(hipMemcpy(kinds.data(), ctx->cell_kind.p, (size_t)ctx->C * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) {
    if (cells[i] < 0 || cells[i] >= ctx->C) return refuse("cell out of range");
    if (kinds[cells[i]] != 1) return refuse("cell is not a solid cell");
  }
  // the bytes of fsi_band_begin with nnode = 4 n DG1 dofs of six components: nrow = 24 n rows
  const std::vector<int32_t> list(cells, cells + n), unused((size_t)n, -1);      // idx0: the cells
  return band_open(ctx, "fsi_band_begin_cells", quantity, 4 * n, 6, capacity, list, unused);
}

int fsi_band_sample(FsiCtx* ctx, int32_t quantity) {
  auto* s = band_entry(ctx, "fsi_band_sample", quantity, ANY_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  if (tensor_quantity(quantity))
    FSICHK(history_append(ctx, s, "fsi_band_sample", "fsi_band_begin_cells", [&](double* dst) {
      launch_tensor_sample(ctx->stream, s->nsamp, elem_arrays(ctx), elem_params(ctx), ctx->U.p, s->idx0.p, quantity == FSI_BAND_STRAIN, dst);
    }));
  else
    FSICHK(history_sample(ctx, s, "fsi_band_sample", "fsi_band_begin"));
  s->frames_changed();
  return FSI_OK;
}

int fsi_band_select(FsiCtx* ctx, int32_t quantity, int64_t first, int64_t count, int64_t stride) {
  auto* s = band_entry(ctx, "fsi_band_select", quantity, ANY_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  const bool fits = stride >= 1 && first >= 0 && first < s->frames && (count == -1 || (count >= 1 && count - 1 <= (s->frames - 1 - first) / stride));
  if (!fits) {
    ctx->err = "fsi_band_select: needs stride >= 1, first >= 0, count >= 1 or -1 and first + (count - 1) * stride < the " +
               std::to_string(s->frames) + " recorded frames";
    return FSI_ERR_INVALID;
  }
  s->sel_first = first;
  s->sel_stride = stride;
  s->sel_count = count == -1 ? (s->frames - 1 - first) / stride + 1 : count;
  s->selection_changed();
  return FSI_OK;
}

int fsi_band_filter(FsiCtx* ctx, int32_t quantity, int32_t ntaps, const double* b, const double* a, const double* zi, int32_t padlen) {
  auto* s = band_entry(ctx, "fsi_band_filter", quantity, ANY_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  FSICHK(history_filter(ctx, s, "fsi_band_filter", "2 .. 11", ntaps, b, a, zi, padlen, raw_view(s, s)));
  s->series_changed();          // the filtered series is the band again: no phase average
  return FSI_OK;
}

int fsi_band_filter_next(FsiCtx* ctx, int32_t quantity, int32_t ntaps, const double* b, const double* a, const double* zi, int32_t padlen) {
  auto* s = band_entry(ctx, "fsi_band_filter_next", quantity, ANY_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  BandCoef c;
  FSICHK(filter_coef(ctx, "fsi_band_filter_next", "2 .. 11", ntaps, b, a, zi, padlen, band_frames(s), &c));
  if (!s->filtered) { ctx->err = "fsi_band_filter_next: no filtered series (fsi_band_filter first)"; return FSI_ERR_INVALID; }
  if (padlen > s->padlen) {     // the stage works inside work: its extension may not reach into the series it is formed from
    ctx->err = "fsi_band_filter_next: padlen = " + std::to_string(padlen) + " after a stage of padlen = " + std::to_string(s->padlen) +
               ": a stage's padlen may not exceed the previous one's (put the longer filter first)";
    return FSI_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(ctx->device));
  launch_band_filter_next(ctx->stream, s->nrow, band_frames(s), s->padlen, padlen, c, s->work.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s->padlen = padlen;
  s->series_changed();          // the series is no longer the fluctuation about the mean
  return FSI_OK;
}

int fsi_band_phase(FsiCtx* ctx, int32_t quantity, int64_t period) {
  auto* s = band_entry(ctx, "fsi_band_phase", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  const SeriesView v = raw_view(s, s);
  const int64_t n = v.frames;
  if (period < 1 || n < 1 || n % period != 0) {
    ctx->err = "fsi_band_phase: period = " + std::to_string(period) + " frames, " + std::to_string(n) +
               " selected frames: needs period >= 1 and a selected count that is a positive multiple of it (fsi_band_select)";
    return FSI_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  // the period's mean frames: those of an earlier call are given back first where they are of another size, and serve again otherwise
  const Want wants[] = {{&s->phase.mean, (size_t)period * (size_t)s->nrow}};
  const bool fresh = !wants[0].stands;
  FSICHK(room_for(ctx, "fsi_band_phase", "the phase means need", counted(s->nrow, " rows x ", period, " frames"), wants, [&] { s->phase.release(); }));
  if (fresh) s->phase.period = 0;
  launch_phase_decompose(ctx->stream, s->nrow, period, n / period, v.x, v.frame_stride / s->nrow, s->phase.mean.p, s->work.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s->series_changed(true);      // the mean frames are this call's own
  s->padlen = 0;                // the fluctuation is the filtered series, without guard frames
  s->filtered = true;
  s->phase.period = period;
  return FSI_OK;
}

int fsi_band_phase_fetch(FsiCtx* ctx, int32_t quantity, int32_t what, int64_t frame, double* out) {
  auto* s = band_entry(ctx, "fsi_band_phase_fetch", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_band_phase_fetch"};
  if (what < FSI_PHASE_MEAN || what > FSI_PHASE_ENERGY_TIME_MEAN) return refuse("what must be FSI_PHASE_MEAN .. FSI_PHASE_ENERGY_TIME_MEAN");
  if (!out) return refuse("out is NULL");
  if (s->phase.period < 1 || !s->filtered) return refuse("no phase average (fsi_band_phase first)");
  if (what != FSI_PHASE_MEAN && s->ncomp != 1 && s->ncomp != 3) return refuse("a strain / stress session has no energy: 0.5 |u'|^2 is that of a vector or a scalar");
  const int64_t P = s->phase.period, n = band_frames(s);
  const int64_t limit = what == FSI_PHASE_ENERGY ? n : what == FSI_PHASE_ENERGY_TIME_MEAN ? 1 : P;
  if (frame < 0 || frame >= limit) return refuse("frame " + std::to_string(frame) + " out of range, this kind has " + std::to_string(limit));
  HIPCHK(hipSetDevice(ctx->device));
  const double* src = nullptr;
  if (what == FSI_PHASE_MEAN) src = s->phase.mean.p + (size_t)frame * s->nrow;
  else {
    const double* f = history_frame(s, true, frame);
    if (what == FSI_PHASE_ENERGY) launch_phase_energy(ctx->stream, s->nnode, s->ncomp, f, 0, 1, false, s->mag.p);
    else if (what == FSI_PHASE_ENERGY_CYCLE_MEAN) launch_phase_energy(ctx->stream, s->nnode, s->ncomp, f, P * s->nrow, n / P, true, s->mag.p);
    else launch_phase_energy(ctx->stream, s->nnode, s->ncomp, f, s->nrow, n, true, s->mag.p);
    HIPCHK(hipGetLastError());
    src = s->mag.p;
  }
  HIPCHK(hipMemcpyAsync(out, src, (size_t)(what == FSI_PHASE_MEAN ? s->nrow : s->nnode) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_band_spi(FsiCtx* ctx, int32_t quantity, const double* window, int64_t bin0, int64_t nb, const double* Ct, const double* St) {
  auto* s = band_entry(ctx, "fsi_band_spi", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_band_spi"};
  if (tensor_quantity(quantity)) return refuse("a strain / stress session has no spectral power index: it is that of a vector or a scalar (d, v, p)");
  const SeriesView v = raw_view(s, s);
  const int64_t n = v.frames, stride = v.frame_stride / s->nrow;
  auto& spi = s->spi;
  if (n < 2) return refuse(std::to_string(n) + " selected frames, the index needs at least 2 (fsi_band_select)");
  if (nb < 1 || bin0 < 0 || !Ct || !St) return refuse("needs bin0 >= 0, nb >= 1 bins and their cos / sin columns Ct, St");
  if (nb - 1 > (n - 1) / 2 - bin0)
    return refuse("bins " + std::to_string(bin0) + " .. " + std::to_string(bin0 + nb - 1) + " of " + std::to_string(n) + " selected frames: a low bin lies below the Nyquist "
                  "frequency, at most bin " + std::to_string((n - 1) / 2));
  if (bin0 > 0 && (spi.next != bin0 || spi.frames != n))
    return refuse("a slab out of order: bin0 = " + std::to_string(bin0) + ", " +
                  (spi.next < 0 ? std::string("no slab stands before it (bin0 = 0 first)") : "the next slab starts at bin " + std::to_string(spi.next)));
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  // the working buffers: those of an earlier call are kept where they have the size, and a larger table serves as well
  const size_t nrow = (size_t)s->nrow;
  const Want wants[] = {{&spi.acc, 3 * nrow}, {&spi.mean, nrow}, {&spi.out, nrow + (size_t)s->nnode}, {&spi.w, (size_t)n}, {&spi.tab, 2 * (size_t)n * (size_t)nb, true}};
  if (bin0 > 0 && !(wants[0].stands && wants[1].stands && wants[2].stands && wants[3].stands))
    return refuse("a slab out of order: the sums of the slabs before it are gone (bin0 = 0 first)");
  FSICHK(room_for(ctx, "fsi_band_spi", "the sums and tables need", std::to_string(s->nrow) + " rows, " + counted(n, " frames x ", nb, " bins of cos and sin"),
                         wants, [&] { spi.release(); }));      // the session stands as before any index was asked for
  double *l2 = spi.acc.p, *x0 = l2 + nrow, *q = x0 + nrow, *Cd = spi.tab.p, *Sd = Cd + (size_t)n * (size_t)nb;
  spi.next = -1;                  // until this slab has run
  spi.closed = false;
  if (bin0 == 0) {
    if (window) HIPCHK(hipMemcpyAsync(spi.w.p, window, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_spec_mean(ctx->stream, s->nrow, n, 0, 1, v.x, spi.mean.p, stride);
  }
  HIPCHK(hipMemcpyAsync(Cd, Ct, (size_t)n * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(Sd, St, (size_t)n * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_spi_power(ctx->stream, s->nrow, n, stride, nb, bin0, v.x, spi.mean.p, window ? spi.w.p : nullptr, Cd, Sd, l2, x0, q);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));                       // the caller's tables are free again
  spi.next = bin0 + nb;
  spi.frames = n;
  return FSI_OK;
}

int fsi_band_spi_fetch(FsiCtx* ctx, int32_t quantity, int32_t what, double* out) {
  auto* s = band_entry(ctx, "fsi_band_spi_fetch", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_band_spi_fetch"};
  auto& spi = s->spi;
  if (what < FSI_SPI_ROWS || what > FSI_SPI_SUMS) return refuse("what must be FSI_SPI_ROWS, FSI_SPI_NODES or FSI_SPI_SUMS");
  if (!out) return refuse("out is NULL");
  if (spi.next < 1) return refuse("no spectral power index (fsi_band_spi first)");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t nrow = (size_t)s->nrow;
  const double* src = spi.acc.p;
  size_t count = 3 * nrow;
  if (what != FSI_SPI_SUMS) {
    if (!spi.closed) {
      launch_spi_close(ctx->stream, s->nnode, s->ncomp, spi.frames, spi.acc.p, spi.acc.p + nrow, spi.acc.p + 2 * nrow, spi.out.p, spi.out.p + nrow);
      HIPCHK(hipGetLastError());
      spi.closed = true;
    }
    src = what == FSI_SPI_ROWS ? spi.out.p : spi.out.p + nrow;
    count = what == FSI_SPI_ROWS ? nrow : (size_t)s->nnode;
  }
  HIPCHK(hipMemcpyAsync(out, src, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_band_pod_gram(FsiCtx* ctx, int32_t quantity, int32_t series, const double* node_weights) {
  auto* s = band_entry(ctx, "fsi_band_pod_gram", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_band_pod_gram"};
  if (tensor_quantity(quantity)) return refuse("a strain / stress session has no proper orthogonal decomposition: it is that of a vector or a scalar (d, v, p)");
  if (series != FSI_RATE_RAW && series != FSI_RATE_SERIES) return refuse("series must be FSI_RATE_RAW or FSI_RATE_SERIES");
  const int64_t n = band_frames(s);
  if (n < 2) return refuse(std::to_string(n) + " selected frames, the decomposition needs at least 2 (fsi_band_select)");
  if (n > POD_MAX_FRAMES) return refuse(std::to_string(n) + " selected frames, the decomposition takes at most " + std::to_string(POD_MAX_FRAMES));
  if (series == FSI_RATE_SERIES && !s->filtered) return refuse("no filtered series (fsi_band_filter or fsi_band_phase first)");
  const size_t nrow = (size_t)s->nrow;
  std::vector<double> hw;                   // the weight of every row's node
  if (node_weights) {
    for (int64_t i = 0; i < s->nnode; ++i)
      if (!(node_weights[i] >= 0.0) || !std::isfinite(node_weights[i])) {
        char msg[160];
        snprintf(msg, sizeof msg, "the weight of node %lld is %g: a weight is >= 0 and finite", (long long)i, node_weights[i]);
        return refuse(msg);
      }
    hw.resize(nrow);
    for (size_t r = 0; r < nrow; ++r) hw[r] = node_weights[r / (size_t)s->ncomp];
  }
  HIPCHK(hipSetDevice(ctx->device));
  // G, the slabs' partial tiles, the mean and the weights; what a decomposition that stands holds, its table and modes included,
  // is given back first - but only once the call is known to fit
  auto& pod = s->pod;
  const Want wants[] = {{&pod.g, (size_t)(n * n)}, {&pod.part, pod_part_count(s->nrow, n)}, {&pod.mean, nrow}, {&pod.w, node_weights ? nrow : 0},
                        {&pod.tab, 0}, {&pod.modes, 0}};
  FSICHK(room_for(ctx, "fsi_band_pod_gram", "the Gram matrix needs",
                         counted(n, " x ", n, " entries, ") + counted(pod_slabs(s->nrow), " slabs x ", pod_pairs(n), " tiles of partial sums, ") +
                             std::to_string(s->nrow) + " rows of means" + (node_weights ? " and weights" : ""),
                         wants, [&] { pod.release(); }, true));
  const SeriesView v = series_view(s, series);
  if (node_weights) HIPCHK(hipMemcpyAsync(pod.w.p, hw.data(), nrow * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_spec_mean(ctx->stream, s->nrow, n, 0, 1, v.x, pod.mean.p, v.frame_stride / s->nrow);
  launch_pod_gram(ctx->stream, s->nrow, n, v.frame_stride, v.x, pod.mean.p, node_weights ? pod.w.p : nullptr, pod.part.p);
  launch_pod_gram_close(ctx->stream, s->nrow, n, pod.part.p, pod.g.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));                       // the host's weights are free again
  pod.source = series;
  pod.frames = n;
  return FSI_OK;
}

int fsi_band_pod_modes(FsiCtx* ctx, int32_t quantity, int32_t nmodes, const double* table) {
  auto* s = band_entry(ctx, "fsi_band_pod_modes", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_band_pod_modes"};
  auto& pod = s->pod;
  if (pod.source < 0) return refuse("no Gram matrix (fsi_band_pod_gram first)");
  if (nmodes < 1 || nmodes > POD_MAX_MODES || !table) return refuse("needs 1 <= nmodes <= " + std::to_string(POD_MAX_MODES) + " modes and their table [frames][nmodes]");
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = pod.frames;
  const size_t ntab = (size_t)n * (size_t)nmodes;
  const Want wants[] = {{&pod.tab, ntab}, {&pod.modes, (size_t)nmodes * (size_t)s->nrow}};      // one count of modes: both stand or neither
  FSICHK(room_for(ctx, "fsi_band_pod_modes", "the modes need", counted(nmodes, " modes x ", s->nrow, " rows and their table of ") + std::to_string(n) + " frames",
                         wants, [&] { pod.tab.release(); pod.modes.release(); pod.nmodes = 0; }));
  const SeriesView v = series_view(s, pod.source);
  pod.nmodes = 0;                   // until the launch has run
  HIPCHK(hipMemcpyAsync(pod.tab.p, table, ntab * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_pod_modes(ctx->stream, s->nrow, n, v.frame_stride, nmodes, v.x, pod.mean.p, pod.tab.p, pod.modes.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));                       // the caller's table is free again
  pod.nmodes = nmodes;
  return FSI_OK;
}

int fsi_band_pod_fetch(FsiCtx* ctx, int32_t quantity, int32_t what, int64_t index, double* out) {
  auto* s = band_entry(ctx, "fsi_band_pod_fetch", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_band_pod_fetch"};
  const auto& pod = s->pod;
  if (what < FSI_POD_GRAM || what > FSI_POD_MODE) return refuse("what must be FSI_POD_GRAM, FSI_POD_MEAN or FSI_POD_MODE");
  if (!out) return refuse("out is NULL");
  if (pod.source < 0) return refuse("no Gram matrix (fsi_band_pod_gram first)");
  const double* src = what == FSI_POD_GRAM ? pod.g.p : pod.mean.p;
  size_t count = what == FSI_POD_GRAM ? (size_t)(pod.frames * pod.frames) : (size_t)s->nrow;
  if (what == FSI_POD_MODE) {
    if (pod.nmodes < 1) return refuse("no modes (fsi_band_pod_modes first)");
    if (index < 0 || index >= pod.nmodes) return refuse("mode " + std::to_string(index) + " out of range, " + std::to_string(pod.nmodes) + " modes stand");
    src = pod.modes.p + (size_t)index * (size_t)s->nrow;
  }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out, src, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_band_cells(FsiCtx* ctx, int32_t quantity, int64_t n, const int32_t* cells, double* grad_out) {
  auto* s = band_entry(ctx, "fsi_band_cells", quantity, WHOLE_CONTEXT | VECTOR_ONLY, ": the strain rate is that of a vector on P2 nodes");
  if (!s) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_band_cells"};
  if (n <= 0 || !cells) return refuse("needs n > 0 cells");
  for (int64_t i = 0; i < n; ++i)
    if (cells[i] < 0 || cells[i] >= ctx->C) return refuse("cell out of range");
  // the session node of every P2 node: the first occurrence of a node that is listed twice
  std::vector<int32_t> at((size_t)ctx->N2, -1);
  for (int64_t i = (int64_t)s->h_nodes.size() - 1; i >= 0; --i)
    if (s->h_nodes[i] >= 0) at[s->h_nodes[i]] = (int32_t)i;
  std::vector<int32_t> conn((size_t)n * 10);
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 10; ++a) {
      const int32_t node = ctx->h_tet_nodes[10 * (int64_t)cells[i] + a];
      if (at[node] < 0)
        return refuse("cell " + std::to_string(cells[i]) + " (entry " + std::to_string(i) + " of the list) has P2 node " + std::to_string(node) +
                      ", which is no node of the session (a session on every P2 node is needed: save_deg 2)");
      conn[10 * i + a] = at[node];
    }
  HIPCHK(hipSetDevice(ctx->device));
  // the list that stands is given back only once the new one is in place, so it counts as taken: the new one is made beside it
  DevBuf<int32_t> d_conn, d_cells;                                 // d_cells: live for this call
  DevBuf<double> d_gl, d_out;
  const Want wants[] = {{&d_conn, (size_t)n * 10}, {&d_gl, (size_t)n * 12}, {&d_out, (size_t)n}};
  FSICHK(room_for(ctx, "fsi_band_cells", "the cell list needs", std::to_string(n) + " cells x 144: ten nodes, twelve gradients, one result", wants, [] {}));
  HIPCHK(d_cells.alloc((size_t)n));
  HIPCHK(hipDeviceSynchronize());                                  // the allocation's own fill is done
  HIPCHK(hipMemcpyAsync(d_conn.p, conn.data(), conn.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(d_cells.p, cells, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  launch_cell_gradients(ctx->stream, n, ctx->geom.p, d_cells.p, d_gl.p);
  HIPCHK(hipGetLastError());
  if (grad_out) HIPCHK(hipMemcpyAsync(grad_out, d_gl.p, (size_t)n * 12 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s->cells.conn.swap(d_conn);      // the earlier list leaves with the locals
  s->cells.gl.swap(d_gl);
  s->cells.out.swap(d_out);
  s->cells.n = n;
  s->cell_list_changed();
  return FSI_OK;
}

int fsi_band_cell_rate(FsiCtx* ctx, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count, double* out) {
  const char* fn = "fsi_band_cell_rate";
  auto* s = cell_series_session(ctx, fn, quantity, series);
  if (!s) return FSI_ERR_INVALID;
  if (!out) return Refusal{ctx, fn}("out is NULL");
  SeriesView x{};
  FSICHK(cell_series_frames(ctx, fn, s, series, first, step, count, &x));
  HIPCHK(hipSetDevice(ctx->device));
  auto& c = s->cells;
  launch_cell_rate(ctx->stream, c.n, c.conn.p, c.gl.p, x.x, x.frame_stride, count, c.out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c.out.p, (size_t)c.n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_band_cell_rate_current(FsiCtx* ctx, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count, double* rate_out,
                               double* volume_ratio_out, double* min_jacobian_out) {
  const char* fn = "fsi_band_cell_rate_current";
  auto* s = cell_series_session(ctx, fn, quantity, series);
  if (!s) return FSI_ERR_INVALID;
  if (!rate_out) return Refusal{ctx, fn}("rate_out is NULL");
  SeriesView x{}, geo{};
  FSICHK(cell_series_frames(ctx, fn, s, series, first, step, count, &x));
  FSICHK(cell_geometry_frames(ctx, fn, s, series, first, step, count, &geo));
  HIPCHK(hipSetDevice(ctx->device));
  auto& c = s->cells;
  const Want wants[] = {{&c.vol, (size_t)c.n, false, false}, {&c.minj, (size_t)c.n, false, false}};      // made together: both stand or neither
  FSICHK(room_for(ctx, fn, "the two further results need", std::to_string(c.n) + " cells x 16", wants, [&] { c.vol.release(); c.minj.release(); }));
  launch_cell_rate_current(ctx->stream, c.n, c.conn.p, c.gl.p, x.x, x.frame_stride, geo.x, geo.frame_stride, count, c.out.p, c.vol.p, c.minj.p);
  HIPCHK(hipGetLastError());
  const size_t bytes = (size_t)c.n * sizeof(double);
  HIPCHK(hipMemcpyAsync(rate_out, c.out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (volume_ratio_out) HIPCHK(hipMemcpyAsync(volume_ratio_out, c.vol.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (min_jacobian_out) HIPCHK(hipMemcpyAsync(min_jacobian_out, c.minj.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_band_cell_weights(FsiCtx* ctx, int32_t quantity, const double* weights) {
  auto* s = band_entry(ctx, "fsi_band_cell_weights", quantity, WHOLE_CONTEXT | VECTOR_ONLY);
  if (!s) return FSI_ERR_INVALID;
  auto& c = s->cells;
  if (c.n < 1) return Refusal{ctx, "fsi_band_cell_weights"}("no cell list (fsi_band_cells first)");
  if (!weights) { c.weighted = false; return FSI_OK; }
  HIPCHK(hipSetDevice(ctx->device));
  FSICHK(cell_buffer(ctx, "fsi_band_cell_weights", "the weights need", &c.weight, (size_t)c.n, std::to_string(c.n) + " cells x 8"));
  HIPCHK(hipMemcpyAsync(c.weight.p, weights, (size_t)c.n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));                       // the caller's array is free again
  c.weighted = true;
  return FSI_OK;
}

int fsi_band_cell_vortex(FsiCtx* ctx, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count, double* cells_out,
                         double* sums_out) {
  return cell_vortex(ctx, "fsi_band_cell_vortex", false, quantity, series, first, step, count, cells_out, sums_out);
}

int fsi_band_cell_vortex_current(FsiCtx* ctx, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count, double* cells_out,
                                 double* sums_out) {
  return cell_vortex(ctx, "fsi_band_cell_vortex_current", true, quantity, series, first, step, count, cells_out, sums_out);
}

int fsi_band_amplitude(FsiCtx* ctx, int32_t quantity, int32_t window) {
  auto* s = band_entry(ctx, "fsi_band_amplitude", quantity, ANY_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  if (!s->filtered) { ctx->err = "fsi_band_amplitude: no filtered series (fsi_band_filter first)"; return FSI_ERR_INVALID; }
  if (window < 0 || window > band_frames(s)) {
    ctx->err = "fsi_band_amplitude: window of " + std::to_string(window) + " frames, the series has " + std::to_string(band_frames(s));
    return FSI_ERR_INVALID;
  }
  s->amplitude_changed(window);
  return FSI_OK;
}

int fsi_band_fetch(FsiCtx* ctx, int32_t quantity, int32_t what, int64_t frame, double* out, double* max_out, int64_t* argmax_out) {
  auto* s = band_entry(ctx, "fsi_band_fetch", quantity, ANY_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  if (what < FSI_BAND_RAW || what > FSI_BAND_MAGNITUDE) { ctx->err = "fsi_band_fetch: what must be FSI_BAND_RAW .. FSI_BAND_MAGNITUDE"; return FSI_ERR_INVALID; }
  if (what != FSI_BAND_RAW && !s->filtered) { ctx->err = "fsi_band_fetch: no filtered series (fsi_band_filter first)"; return FSI_ERR_INVALID; }
  // a raw frame keeps its index in the history; the filtered series and the amplitude have the selected frames
  if (frame < 0 || frame >= (what == FSI_BAND_RAW ? s->frames : band_frames(s))) { ctx->err = "fsi_band_fetch: frame out of range"; return FSI_ERR_INVALID; }
  if (what >= FSI_BAND_AMPLITUDE && s->window < 0) { ctx->err = "fsi_band_fetch: no amplitude (fsi_band_amplitude first)"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  const double* src = nullptr;
  if (what == FSI_BAND_RAW) src = history_frame(s, false, frame);
  else if (what == FSI_BAND_FILTERED || s->window == 0) src = history_frame(s, true, frame);   // low-pass: the amplitude is the series (:222-230)
  else {
    // calculate_windowed_rms: RMS[i - pad] for pad <= i < pad + n - w + 1 with pad = (n - len_RMS) // 2, zero outside.  The
    // value of a frame does not depend on the order of the fetches: window `start` is recomputed when start is a multiple of
    // BAND_RMS_REFRESH and advanced from start - 1 otherwise.
    const int64_t w = s->window, n = band_frames(s), start = frame - (w - 1) / 2;
    if (start < 0 || start + w > n) {
      HIPCHK(hipMemsetAsync(s->amp.p, 0, (size_t)s->nrow * sizeof(double), ctx->stream));
    } else {
      int64_t from = start - start % BAND_RMS_REFRESH;
      if (s->acc_start >= from && s->acc_start < start) from = s->acc_start + 1;
      else if (s->acc_start == start) from = start - start % BAND_RMS_REFRESH;     // asked twice: the same arithmetic again
      for (int64_t k = from; k <= start; ++k)
        launch_band_rms(ctx->stream, s->nrow, history_frame(s, true, 0), k, (int)w, k % BAND_RMS_REFRESH == 0, s->acc.p, s->amp.p);
      HIPCHK(hipGetLastError());
      s->acc_start = start;
    }
    src = s->amp.p;
  }
  const bool to_board = what >= FSI_BAND_AMPLITUDE && s->board_node0 >= 0;      // fsi_band_board_attach
  if (to_board && frame >= ctx->board.frames) { ctx->err = "fsi_band_fetch: the attached board has " + std::to_string(ctx->board.frames) + " frames"; return FSI_ERR_INVALID; }
  if (what == FSI_BAND_MAGNITUDE || max_out || argmax_out || to_board) {
    if (what < FSI_BAND_AMPLITUDE) { ctx->err = "fsi_band_fetch: maximum / argmax are those of the amplitude magnitude"; return FSI_ERR_INVALID; }
    if (tensor_quantity(quantity)) launch_tensor_principal(ctx->stream, s->nnode, src, s->mag.p);      // window 0: of the series itself (:229-230)
    else launch_band_magnitude(ctx->stream, s->nnode, s->ncomp, src, s->mag.p);
    if (what == FSI_BAND_MAGNITUDE || max_out || argmax_out) launch_band_argmax(ctx->stream, s->nnode, s->mag.p, s->part_val.p, s->part_idx.p);
    HIPCHK(hipGetLastError());
    if (to_board)
      HIPCHK(hipMemcpyAsync(ctx->board.data.p + (size_t)frame * (size_t)ctx->board.nodes + (size_t)s->board_node0, s->mag.p,
                            (size_t)s->nnode * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (max_out) HIPCHK(hipMemcpyAsync(max_out, s->part_val.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (argmax_out) HIPCHK(hipMemcpyAsync(argmax_out, s->part_idx.p, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (what == FSI_BAND_MAGNITUDE) src = s->mag.p;
  }
  if (out) HIPCHK(hipMemcpyAsync(out, src, (size_t)(what == FSI_BAND_MAGNITUDE ? s->nnode : s->nrow) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_band_trace(FsiCtx* ctx, int32_t quantity, int32_t what, int64_t npoints, const int32_t* points, double* out) {
  auto* s = band_entry(ctx, "fsi_band_trace", quantity, ANY_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  if (tensor_quantity(quantity)) {      // the reference writes no point traces for these quantities (create_hi_pass_viz.py:636-643)
    ctx->err = "fsi_band_trace: a strain / stress session has no point traces";
    return FSI_ERR_INVALID;
  }
  if (what != FSI_BAND_RAW && what != FSI_BAND_FILTERED) { ctx->err = "fsi_band_trace: what must be FSI_BAND_RAW or FSI_BAND_FILTERED"; return FSI_ERR_INVALID; }
  if (npoints <= 0 || !points || !out) { ctx->err = "fsi_band_trace: needs npoints > 0 points and an output"; return FSI_ERR_INVALID; }
  if (what == FSI_BAND_FILTERED && !s->filtered) { ctx->err = "fsi_band_trace: no filtered series (fsi_band_filter first)"; return FSI_ERR_INVALID; }
  for (int64_t i = 0; i < npoints; ++i)
    if (points[i] < 0 || points[i] >= s->nnode) { ctx->err = "fsi_band_trace: node out of range"; return FSI_ERR_INVALID; }
  const int64_t frames = band_frames(s);
  if (frames < 1) { ctx->err = "fsi_band_trace: no recorded frames"; return FSI_ERR_INVALID; }
  const size_t nout = (size_t)npoints * (size_t)frames * (size_t)(1 + s->ncomp);
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf<int32_t> pts;          // live for this call
  DevBuf<double> res;
  HIPCHK(pts.alloc((size_t)npoints));
  HIPCHK(res.alloc(nout));
  HIPCHK(hipDeviceSynchronize());                                  // the allocations' own fills are done
  HIPCHK(hipMemcpyAsync(pts.p, points, (size_t)npoints * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  const SeriesView v = series_view(s, what == FSI_BAND_RAW ? FSI_RATE_RAW : FSI_RATE_SERIES);
  launch_band_trace(ctx->stream, s->nrow, s->ncomp, npoints, pts.p, frames, v.x, v.frame_stride / s->nrow, res.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, res.p, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_band_export(FsiCtx* ctx, int32_t quantity, int64_t first, int64_t count, double* out) {
  auto* s = band_entry(ctx, "fsi_band_export", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  return history_export(ctx, s, "fsi_band_export", first, count, out);
}

int fsi_band_import(FsiCtx* ctx, int32_t quantity, int64_t count, const double* frames) {
  auto* s = band_entry(ctx, "fsi_band_import", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  FSICHK(history_import(ctx, s, "fsi_band_import", count, frames));
  s->frames_changed();
  return FSI_OK;
}

int fsi_band_room(FsiCtx* ctx, int64_t rows, int64_t capacity, double* need, double* available) {
  if (!ctx) return FSI_ERR_INVALID;
  if (rows < 1 || capacity < 1 || !need || !available) { ctx->err = "fsi_band_room: needs rows >= 1, capacity >= 1 and both outputs"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  Room room;
  FSICHK(device_room(ctx, &room));
  *need = band_need(rows, capacity);
  *available = room.available();
  return FSI_OK;
}

int fsi_board_begin(FsiCtx* ctx, int64_t nodes, int64_t frames) {
  if (!ctx) return FSI_ERR_INVALID;
  if (nodes < 1 || frames < 1) { ctx->err = "fsi_board_begin: needs nodes >= 1 and frames >= 1"; return FSI_ERR_INVALID; }
  if (nodes >= (1ll << 32)) { ctx->err = "fsi_board_begin: more than 2^32 - 1 nodes"; return FSI_ERR_INVALID; }
  if (partitioned(ctx, "fsi_board_begin")) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  FSICHK(room_for(ctx, "fsi_board_begin", "the board needs", 8.0 * (double)nodes * (double)frames, counted(nodes, " nodes x ", frames, " frames")));
  for (auto& s : ctx->band) s.board_node0 = -1;      // only now: a refused begin leaves an open board and its sessions as they were
  auto& b = ctx->board;
  b.release();
  HIPCHK(b.data.alloc((size_t)nodes * (size_t)frames));
  HIPCHK(b.part_val.alloc(BAND_ARGMAX_BLOCKS + 1));
  HIPCHK(b.part_idx.alloc(BAND_ARGMAX_BLOCKS + 1));
  HIPCHK(hipDeviceSynchronize());                                  // the allocations' own fills are done
  b.nodes = nodes; b.frames = frames; b.open = true;
  return FSI_OK;
}

int fsi_board_end(FsiCtx* ctx) {
  if (!ctx) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (auto& s : ctx->band) s.board_node0 = -1;
  ctx->board.release();
  return FSI_OK;
}

int fsi_band_board_attach(FsiCtx* ctx, int32_t quantity, int64_t node0) {
  auto* s = band_entry(ctx, "fsi_band_board_attach", quantity, WHOLE_CONTEXT);
  if (!s) return FSI_ERR_INVALID;
  if (node0 == -1) { s->board_node0 = -1; return FSI_OK; }
  if (!ctx->board.open) { ctx->err = "fsi_band_board_attach: no board (fsi_board_begin first)"; return FSI_ERR_INVALID; }
  if (node0 < 0 || node0 > ctx->board.nodes - s->nnode) {
    ctx->err = "fsi_band_board_attach: nodes " + std::to_string(node0) + " .. " + std::to_string(node0) + " + " + std::to_string(s->nnode) +
               " of the session do not lie in the board's " + std::to_string(ctx->board.nodes);
    return FSI_ERR_INVALID;
  }
  s->board_node0 = node0;
  return FSI_OK;
}

int fsi_board_table(FsiCtx* ctx, int64_t first, int64_t count, int32_t nranks, const int64_t* ranks, double* values, int64_t* nan_counts,
                    double* max_out, int64_t* argmax_out) {
  if (!ctx) return FSI_ERR_INVALID;
  if (partitioned(ctx, "fsi_board_table")) return FSI_ERR_INVALID;
  auto& b = ctx->board;
  if (!b.open) { ctx->err = "fsi_board_table: no board (fsi_board_begin first)"; return FSI_ERR_INVALID; }
  if (first < 0 || count < 1 || first > b.frames - count) {
    ctx->err = "fsi_board_table: needs first >= 0, count >= 1 and first + count <= the board's " + std::to_string(b.frames) + " frames";
    return FSI_ERR_INVALID;
  }
  if (!values || !nan_counts || !max_out || !argmax_out) { ctx->err = "fsi_board_table: null output"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  const double* x = b.data.p + (size_t)first * (size_t)b.nodes;
  FSICHK(order_statistics(ctx, "fsi_board_table", b.nodes, count, b.nodes, x, nranks, ranks, values, nan_counts));
  for (int64_t k = 0; k < count; ++k) {      // the frame's maximum and the first node that has it, as fsi_band_fetch forms them
    launch_band_argmax(ctx->stream, b.nodes, x + (size_t)k * (size_t)b.nodes, b.part_val.p, b.part_idx.p);
    HIPCHK(hipMemcpyAsync(max_out + k, b.part_val.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(argmax_out + k, b.part_idx.p, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_order_statistics(FsiCtx* ctx, int64_t n, const double* values, int32_t nranks, const int64_t* ranks, double* out, int64_t* nan_count) {
  if (!ctx) return FSI_ERR_INVALID;
  if (partitioned(ctx, "fsi_order_statistics")) return FSI_ERR_INVALID;
  if (n < 1 || n >= (1ll << 32) || !values || !out || !nan_count) {
    ctx->err = "fsi_order_statistics: needs 1 <= n < 2^32 values, an output and a NaN count";
    return FSI_ERR_INVALID;
  }
  FSICHK(ranks_checked(ctx, "fsi_order_statistics", n, nranks, ranks, nullptr, nullptr));      // before anything is allocated
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf<double> x;             // live for this call
  HIPCHK(x.alloc((size_t)n));
  HIPCHK(hipDeviceSynchronize());                                  // the allocation's own fill is done
  HIPCHK(hipMemcpyAsync(x.p, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return order_statistics(ctx, "fsi_order_statistics", n, 1, n, x.p, nranks, ranks, out, nan_count);
}

int fsi_band_end(FsiCtx* ctx, int32_t quantity) {
  if (!ctx) return FSI_ERR_INVALID;
  return end_session(ctx, ctx->band, quantity, "fsi_band_end");
}

int fsi_spec_begin(FsiCtx* ctx, int32_t quantity, int64_t n, const int32_t* nodes, const int32_t* nodes_b, int32_t ncomp_mode, int64_t capacity) {
  if (!ctx) return FSI_ERR_INVALID;
  int mode = ncomp_mode;
  std::vector<int32_t> i0, i1;
  FSICHK(row_lists(ctx, "fsi_spec_begin", quantity, n, nodes, nodes_b, capacity, &mode, false, i0, i1));
  return spec_open(ctx, "fsi_spec_begin", quantity, n, mode == FSI_SPEC_MAG ? n : (int64_t)i0.size(), mode, capacity, i0, i1);
}

int fsi_spec_begin_rows(FsiCtx* ctx, int32_t quantity, int64_t nrows, const int32_t* nodes, const int32_t* nodes_b, const int32_t* comps,
                        int64_t capacity) {
  if (!ctx) return FSI_ERR_INVALID;
  if (quantity >= 0 && quantity < 2 && !comps) { ctx->err = "fsi_spec_begin_rows: needs the component of every row of d or v"; return FSI_ERR_INVALID; }
  int mode = FSI_SPEC_X;        // one entry per row: comps[r] of nodes[r]
  std::vector<int32_t> i0, i1;
  FSICHK(row_lists(ctx, "fsi_spec_begin_rows", quantity, nrows, nodes, nodes_b, capacity, &mode, false, i0, i1, comps));
  return spec_open(ctx, "fsi_spec_begin_rows", quantity, nrows, nrows, mode, capacity, i0, i1);
}

int fsi_spec_begin_wss(FsiCtx* ctx, int64_t nf, const int32_t* facet_cells, const int32_t* facet_local, double mu, int64_t nrows,
                       const int32_t* dofs, const int32_t* comps, int64_t capacity) {
  if (!ctx) return FSI_ERR_INVALID;
  const Refusal refuse{ctx, "fsi_spec_begin_wss"};
  if (ctx->part) return refuse("partitioned contexts are not supported");
  if (nf <= 0 || !facet_cells || !facet_local || !(mu > 0.0)) return refuse("needs nf > 0 facets and mu > 0");
  if (nf > (int64_t)2147483647 / 3) return refuse("more than 2^31 - 1 dofs on the boundary mesh");
  if (nrows < 1 || !dofs || !comps) return refuse("needs nrows >= 1 rows, the dof and the component of each");
  if (nrows > (int64_t)2147483647 / 2) return refuse("more than 2^30 rows");
  if (capacity < 1) return refuse("needs a capacity >= 1 frames");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<int32_t> kinds((size_t)ctx->C);      // as fsi_stress_begin: range and kind on the host, before anything is uploaded
  HIPCHK(hipMemcpy(kinds.data(), ctx->cell_kind.p, (size_t)ctx->C * sizeof(int32_t), hipMemcpyDeviceToHost));
  // the full exterior-facet mask of every boundary cell, from the whole facet list (as fsi_hemo_begin forms it)
  std::vector<std::pair<int32_t, int32_t>> cellmask;     // (cell, mask), ascending in the cell
  {
    std::vector<std::pair<int32_t, int32_t>> order((size_t)nf);
    for (int64_t f = 0; f < nf; ++f) {
      if (facet_cells[f] < 0 || facet_cells[f] >= ctx->C || facet_local[f] < 0 || facet_local[f] > 3) return refuse("facet cell / local index out of range");
      if (kinds[facet_cells[f]] != 0) return refuse("a facet's cell is not a fluid cell");
      order[f] = {facet_cells[f], facet_local[f]};
    }
    std::sort(order.begin(), order.end());
    for (int64_t k = 0; k < nf; ++k) {
      if (k == 0 || order[k].first != order[k - 1].first) cellmask.push_back({order[k].first, 0});
      if (cellmask.back().second & (1 << order[k].second)) return refuse("a facet is listed twice");
      cellmask.back().second |= 1 << order[k].second;
    }
  }
  // the touched cells in ascending order, and per cell its rows in row order: (row, 4 * local vertex + component)
  static const int VERTS[4][3] = {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}};
  int64_t nmag = 0;
  std::vector<std::pair<int32_t, int64_t>> by_cell((size_t)nrows);      // (cell, row)
  for (int64_t r = 0; r < nrows; ++r) {
    if (dofs[r] < 0 || dofs[r] >= 3 * nf) return refuse("dof out of range, needs 0 <= dof < 3 nf");
    if (comps[r] < 0 || comps[r] > 3) return refuse("component out of range, needs 0 (x), 1 (y), 2 (z) or 3 (magnitude)");
    nmag += comps[r] == 3;
    by_cell[r] = {facet_cells[dofs[r] / 3], r};
  }
  std::sort(by_cell.begin(), by_cell.end());
  std::vector<int32_t> ucell, mask, ptr, ent((size_t)(2 * nrows));
  for (int64_t k = 0; k < nrows; ++k) {
    const int64_t r = by_cell[k].second;
    if (k == 0 || by_cell[k].first != by_cell[k - 1].first) {
      const auto it = std::lower_bound(cellmask.begin(), cellmask.end(), std::make_pair(by_cell[k].first, (int32_t)0));
      ucell.push_back(by_cell[k].first);
      mask.push_back(it->second);
      ptr.push_back((int32_t)k);
    }
    ent[2 * k] = (int32_t)r;
    ent[2 * k + 1] = 4 * VERTS[facet_local[dofs[r] / 3]][dofs[r] % 3] + comps[r];
  }
  ptr.push_back((int32_t)nrows);
  FSICHK(spec_room_for(ctx, "fsi_spec_begin_wss", nrows, nrows + 2 * nmag, capacity));      // a magnitude row as in fsi_spec_room
  auto& s = ctx->spec[FSI_SPEC_WSS];
  s.release();                  // only now: a refused begin leaves an open session of the quantity as it was
  s.mode = FSI_SPEC_X;
  s.mu = mu;
  s.wncell = (int64_t)ucell.size();
  s.nnode = s.nrow = s.nsamp = nrows;
  s.capacity = capacity;
  HIPCHK(s.wcells.alloc(ucell.size()));
  HIPCHK(s.wmask.alloc(mask.size()));
  HIPCHK(s.wptr.alloc(ptr.size()));
  HIPCHK(s.went.alloc(ent.size()));
  HIPCHK(s.hist.alloc((size_t)nrows * (size_t)capacity));
  HIPCHK(s.work.alloc((size_t)nrows * (size_t)(capacity + 2 * BAND_MAX_PADLEN)));
  HIPCHK(hipDeviceSynchronize());                                  // the allocations' own fills are done
  HIPCHK(hipMemcpyAsync(s.wcells.p, ucell.data(), ucell.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(s.wmask.p, mask.data(), mask.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(s.wptr.p, ptr.data(), ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(s.went.p, ent.data(), ent.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s.open = true;
  return FSI_OK;
}

int fsi_spec_room(FsiCtx* ctx, int64_t rows, int32_t magnitude, int64_t capacity, double* need, double* available) {
  if (!ctx) return FSI_ERR_INVALID;
  if (rows < 1 || capacity < 1 || !need || !available) { ctx->err = "fsi_spec_room: needs rows >= 1, capacity >= 1 and both outputs"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  Room room;
  FSICHK(device_room(ctx, &room));
  *need = spec_need(rows, magnitude ? 3 * rows : rows, capacity);
  *available = room.available();
  return FSI_OK;
}

int fsi_spec_sample(FsiCtx* ctx, int32_t quantity) {
  if (!ctx) return FSI_ERR_INVALID;
  auto* s = spec_session(ctx, quantity, "fsi_spec_sample");
  if (!s) return FSI_ERR_INVALID;
  if (quantity != FSI_SPEC_WSS) return history_sample(ctx, s, "fsi_spec_sample", "fsi_spec_begin");
  return history_append(ctx, s, "fsi_spec_sample", "fsi_spec_begin_wss", [&](double* dst) {
    launch_spec_wss_sample(ctx->stream, s->wncell, elem_arrays(ctx), ctx->U.p, s->wcells.p, s->wmask.p, s->wptr.p, s->went.p, s->mu, dst);
  });
}

int fsi_spec_filter(FsiCtx* ctx, int32_t quantity, int32_t ntaps, const double* b, const double* a, const double* zi, int32_t padlen) {
  if (!ctx) return FSI_ERR_INVALID;
  auto* s = spec_session(ctx, quantity, "fsi_spec_filter");
  if (!s) return FSI_ERR_INVALID;
  if (ntaps == 0) { s->filtered = false; return FSI_OK; }      // back to the raw series
  return history_filter(ctx, s, "fsi_spec_filter", "0 (the raw series) or 2 .. 11", ntaps, b, a, zi, padlen, SeriesView{s->hist.p, s->frames, s->nrow});
}

int fsi_spec_fetch(FsiCtx* ctx, int32_t quantity, int32_t filtered, int64_t frame, double* out) {
  if (!ctx) return FSI_ERR_INVALID;
  auto* s = spec_session(ctx, quantity, "fsi_spec_fetch");
  if (!s) return FSI_ERR_INVALID;
  if (!out) { ctx->err = "fsi_spec_fetch: out is NULL"; return FSI_ERR_INVALID; }
  if (filtered && !s->filtered) { ctx->err = "fsi_spec_fetch: no filtered series (fsi_spec_filter first)"; return FSI_ERR_INVALID; }
  if (frame < 0 || frame >= s->frames) { ctx->err = "fsi_spec_fetch: frame out of range"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out, history_frame(s, filtered != 0, frame), (size_t)s->nrow * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_spec_spectrogram(FsiCtx* ctx, int32_t quantity, int64_t nperseg, int64_t noverlap, int64_t nfft, const double* window,
                         int32_t scaling, double fs, double* out_power) {
  return spec_transform(ctx, "fsi_spec_spectrogram", false, quantity, nperseg, noverlap, nfft, window, scaling, fs, out_power, false, 0, 0);
}

int fsi_spec_periodogram(FsiCtx* ctx, int32_t quantity, const double* window, int32_t scaling, double fs, double* out_power) {
  return spec_transform(ctx, "fsi_spec_periodogram", true, quantity, 0, 0, 0, window, scaling, fs, out_power, false, 0, 0);
}

int fsi_spec_spectrogram_sum(FsiCtx* ctx, int32_t quantity, int64_t nperseg, int64_t noverlap, int64_t nfft, const double* window,
                             int32_t scaling, double fs, int64_t first_row, int64_t total_rows, double* carry) {
  return spec_transform(ctx, "fsi_spec_spectrogram_sum", false, quantity, nperseg, noverlap, nfft, window, scaling, fs, carry, true, first_row, total_rows);
}

int fsi_spec_periodogram_sum(FsiCtx* ctx, int32_t quantity, const double* window, int32_t scaling, double fs, int64_t first_row,
                             int64_t total_rows, double* carry) {
  return spec_transform(ctx, "fsi_spec_periodogram_sum", true, quantity, 0, 0, 0, window, scaling, fs, carry, true, first_row, total_rows);
}

int fsi_spec_export(FsiCtx* ctx, int32_t quantity, int64_t first, int64_t count, double* out) {
  if (!ctx) return FSI_ERR_INVALID;
  if (partitioned(ctx, "fsi_spec_export")) return FSI_ERR_INVALID;
  auto* s = spec_session(ctx, quantity, "fsi_spec_export");
  if (!s) return FSI_ERR_INVALID;
  return history_export(ctx, s, "fsi_spec_export", first, count, out);
}

int fsi_spec_import(FsiCtx* ctx, int32_t quantity, int64_t count, const double* frames) {
  if (!ctx) return FSI_ERR_INVALID;
  if (partitioned(ctx, "fsi_spec_import")) return FSI_ERR_INVALID;
  auto* s = spec_session(ctx, quantity, "fsi_spec_import");
  if (!s) return FSI_ERR_INVALID;
  return history_import(ctx, s, "fsi_spec_import", count, frames);      // filtered = false: the raw series is selected
}

int fsi_spec_end(FsiCtx* ctx, int32_t quantity) {
  if (!ctx) return FSI_ERR_INVALID;
  return end_session(ctx, ctx->spec, quantity, "fsi_spec_end");
}

}  // extern "C"
