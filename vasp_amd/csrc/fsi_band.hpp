// Band-pass filtered fields and vibration amplitudes of a run (fsi_band.hip): sizes, the filter's coefficients as a kernel
// argument, and the launchers the C-ABI (fsi_band_* in fsi_sessions.hip) calls.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fsi {

constexpr int BAND_MAX_TAPS = 11;                      // order-5 band-pass: len(b) = len(a) = 11 (low-pass: 6)
constexpr int BAND_MAX_PADLEN = 3 * BAND_MAX_TAPS;     // scipy's default padlen = 3 max(len(a), len(b))
constexpr int BAND_RMS_REFRESH = 64;                   // the running sum of squares is recomputed exactly every 64 windows

// b, a (a[0] = 1) and lfilter_zi, zero-padded to the largest filter: a zero tap adds x * 0 - y * 0 to the state behind it,
// which changes no value (at most the sign of a zero)
struct BandCoef {
  double b[BAND_MAX_TAPS], a[BAND_MAX_TAPS], zi[BAND_MAX_TAPS - 1];
};

// hist[frame][row] <- the rows of the resident state: U[idx0[row]], or 0.5 * (U[idx0[row]] + U[idx1[row]]) where idx1 >= 0
void launch_band_sample(hipStream_t st, int64_t nrow, const double* U, const int32_t* idx0, const int32_t* idx1, double* dst);
// scipy.signal.filtfilt(b, a, hist[::stride, row]) of every row over nframes frames, the first at hist, into
// work[padlen + frame][row]; work has nframes + 2 padlen frames
void launch_band_filter(hipStream_t st, int64_t nrow, int64_t nframes, int padlen, const BandCoef& c, const double* hist,
                        int64_t stride, double* work);
// the same of the filtered series itself, in place: work[padlen_prev + frame][row] -> work[padlen + frame][row]; needs
// padlen <= padlen_prev (the head of the extension is written below the series it is formed from)
void launch_band_filter_next(hipStream_t st, int64_t nrow, int64_t nframes, int padlen_prev, int padlen, const BandCoef& c, double* work);
// out[point][frame][1 + ncomp] = |.|, then the ncomp values of node points[point] in frame src[frame * stride][.]; a frame
// is [nrow / ncomp][ncomp].  |.| = sqrt((x x + y y) + z z), for ncomp 1 the value itself
void launch_band_trace(hipStream_t st, int64_t nrow, int ncomp, int64_t npoints, const int32_t* points, int64_t nframes,
                       const double* src, int64_t stride, double* out);
// amp[row] = sqrt(sum of y[start .. start + window - 1][row]^2 / window); the sum is recomputed (recompute) or advanced from
// the window that started one frame earlier (acc)
void launch_band_rms(hipStream_t st, int64_t nrow, const double* y, int64_t start, int window, bool recompute, double* acc,
                     double* amp);
// mag[node] = |amp[node][0..2]| (ncomp 3) or amp[node] (ncomp 1); then its maximum and the first node that has it
void launch_band_magnitude(hipStream_t st, int64_t nnode, int ncomp, const double* amp, double* mag);
constexpr int BAND_ARGMAX_BLOCKS = 256;
void launch_band_argmax(hipStream_t st, int64_t n, const double* mag, double* part_val, int64_t* part_idx);   // result in part_*[0]
// Exact order statistics: out[frame][k] = the element of rank ranks[k] (0 = the smallest) of x[frame * stride + 0 .. n), for
// nframes frames; ranks[nranks] on the device, ascending and distinct, nranks <= BAND_SEL_MAX_RANKS, n < 2^32.  nans[frame]:
// the frame's NaNs, which order behind +inf.  Integer counts only: the same call gives the same bits.
constexpr int BAND_SEL_MAX_RANKS = 32;
void launch_band_select(hipStream_t st, int64_t n, int64_t nframes, int64_t stride, const double* x, int nranks, const int64_t* ranks,
                        double* out, int64_t* nans);

}  // namespace fsi
