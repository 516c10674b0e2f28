// The text of a refusal under the room rule of the post-processing sessions (fsi_sessions.hip: room_for): an allocation of
// `need` bytes that does not fit beside the 1/16 of the device the context keeps.  Plain C++, read by the test shim too; the
// texts are part of the interface - callers and tests read the three byte counts back out of them.
#pragma once
#include <cstdio>
#include <string>

namespace fsi {
namespace host {

inline std::string bytes_text(double x) {      // "%.0f": 309 digits at the most
  char buf[336];
  snprintf(buf, sizeof buf, "%.0f", x);
  return buf;
}

// "<fn>: <subject> <need> bytes (<layout>), the device has <free_b> bytes free of which <reserve> stay with the context";
// subject comes with its verb ("the session needs", "the phase means need"), layout says what the bytes are.  Of the proper
// orthogonal decomposition: fsi_band_pod_gram "the Gram matrix needs" with "<n> x <n> entries, <slabs> slabs x <pairs> tiles of
// partial sums, <rows> rows of means[ and weights]", fsi_band_pod_modes "the modes need" with "<nmodes> modes x <rows> rows and
// their table of <n> frames"
inline std::string room_refusal(const std::string& fn, const std::string& subject, double need, const std::string& layout, size_t free_b,
                                double reserve) {
  return fn + ": " + subject + " " + bytes_text(need) + " bytes (" + layout + "), the device has " + std::to_string(free_b) +
         " bytes free of which " + bytes_text(reserve) + " stay with the context";
}

}  // namespace host
}  // namespace fsi
