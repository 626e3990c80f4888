// onset-track.hpp — NOT in the reference (it draws a tempo grid, app.cpp:561-573, and leaves the timing to the mouse): the
// build-defined onset detector (mx_onset_flux, mx_onset_pick) and the markers that move the onsets onto the tempo grid
// (mx_timing_markers), the tempo and grid offset estimated from the onset strength (mx_tempo_from_flux), as a class the App can own next to its melonix::PitchTrack.
//
//   melonix::OnsetTrack onsets(wavData, sampleRate);            // uploads once, onset strength of every frame (hop 256) on the GPU
//   mx_timing_params tp = onsets.timingParams();  tp.bpm = tempo; // the Tempo slider's value ...
//   auto t = onsets.tempo();  tp.bpm = t.bpm; tp.offset = t.offset; // ... or "detect tempo": the grid from the take itself
//   markers = onsets.timingMarkers(tp);                            // "Auto-correct timing": every onset onto the grid ...
//   markers = onsets.timingMarkers(tp, track.correctionMarkers(1.f, 0));   // ... or timing and pitch in one list
//   invalidateCache();                                             // and exportWav / renderPV / renderPSOLA follow dTime
#pragma once
#include <cstdint>
#include <span>
#include <vector>

#include "marker.hpp"
#include "melonix_amd.h"

namespace melonix {

class OnsetTrack {
public:
  // hop: samples between frame centres.  The flux parameters are the library's defaults.
  OnsetTrack(std::span<const float> wav, int sampleRate, int hop = 256, int device = 0);

  bool ok() const { return good; }
  int hop() const { return hop_; }
  // the onset strength of frame h (centred on sample h * hop); empty after a failed call
  const std::vector<float> &flux() const { return flux_; }
  // the defaults (mx_onset_pick_params_default, mx_timing_params_default), to edit and pass on
  static mx_onset_pick_params pickParams();
  static mx_timing_params timingParams();
  // the onsets picked from flux(); empty after a failed call
  std::vector<mx_onset> onsets() const { return onsets(pickParams()); }
  std::vector<mx_onset> onsets(const mx_onset_pick_params &p) const;
  // the markers that put onsets() on the grid; baseMarkers: what PitchTrack::correctionMarkers gives (their bends and notes
  // are kept, the bend over the source is unchanged).  Empty after a failed call.
  std::vector<Marker> timingMarkers(const mx_timing_params &p, const std::vector<Marker> &baseMarkers = {}) const;
  // tempo and grid offset estimated from flux() (mx_tempo_from_flux; bpm 0: no pulse in an empty or silent take), and the
  // per-window tempo curve for display.  Zeroed / empty after a failed call.
  static mx_tempo_params tempoParams();
  mx_tempo tempo() const { return tempo(tempoParams()); }
  mx_tempo tempo(const mx_tempo_params &p) const;
  std::vector<mx_tempo_window> tempoWindows() const { return tempoWindows(tempoParams()); }
  std::vector<mx_tempo_window> tempoWindows(const mx_tempo_params &p) const;
  // both from one run of the estimate (tempo() and tempoWindows() each run it): -> whether it succeeded; windows may be null
  bool estimate(const mx_tempo_params &p, mx_tempo &t, std::vector<mx_tempo_window> *windows) const;

private:
  int sampleRate, hop_, device_;
  int64_t n_;
  bool good = false;
  std::vector<float> flux_;
};

}  // namespace melonix
