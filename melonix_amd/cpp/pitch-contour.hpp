// pitch-contour.hpp — NOT in the reference (it has no such operation): the build-defined pitch-drift and vibrato controls of
// auto-correct (mx_pitch_contour, mx_contour_vibrato, mx_contour_bend, mx_psola_render_bend) as a class the App can own next
// to its melonix::PitchTrack and melonix::KeyTrack.  It wants what PSOLA wants: a monophonic take.
//
//   melonix::PitchContour contour(wavData, sampleRate);     // uploads once: decoded f0 track, notes, the split, the figures
//   // per note: contour.vibrato()[i].rate_hz / .extent_cents / .strength / .drift_cents, for the note's inspector
//   pcm = contour.correct(1.f, 0.5f, shift);                // drift removed, vibrato halved, note i moved by shift[i] semitones
//   // shift: e.g. key.correctionMarkers(contour.notes(), 1.f)[2 * i].pitchBend — then pass no markers, or the bend comes twice
#pragma once
#include <cstdint>
#include <span>
#include <vector>

#include "marker.hpp"
#include "melonix_amd.h"

namespace melonix {

class PitchContour {
public:
  // hop: samples between frame centres.  The track is the Viterbi-decoded one (mx_f0_track_decoded, the tracker's and the
  // decoder's defaults); notes, contour and renders read it with the voicing threshold melonix::PitchTrack uses for a decoded
  // track (2 x 0.15).  The split's parameters are mx_contour_params_default(sampleRate, hop).
  PitchContour(std::span<const float> wav, int sampleRate, int hop = 256, int device = 0);

  bool ok() const { return good; }
  int hop() const { return hop_; }
  // everything below is empty after a failed construction
  const std::vector<mx_f0> &frames() const { return track; }            // one record per frame h (centred on sample h * hop)
  const std::vector<mx_note> &notes() const { return notes_; }
  const std::vector<mx_contour_rec> &contour() const { return rec; }    // per frame: smooth (centre + drift) and vibrato
  const std::vector<mx_contour_stat> &stats() const { return stat; }    // per note
  const std::vector<mx_vibrato> &vibrato() const { return vibrato_; }   // per note: rate, extent, strength, drift
  // the bend curve, semitones per frame: drift in [0, 1] (1 removes it), vibrato in [0, 4] (0 removes it, 1 leaves it, 2 doubles
  // it), shift one value per note or none, glideFrames the longest gap between notes the curve is carried across.  Empty
  // after a failed call (parameters out of range, a shift that is not finite or not one per note).
  std::vector<float> bend(float drift, float vibrato, std::span<const double> shift = {}, int glideFrames = 8) const;
  // the take rendered along that curve by PSOLA (formants in place; `points` move them), float PCM of
  // mx_pv_render_length(n, sr, markers) samples; the markers' own time map and bend apply on top.  Empty after a failed call.
  std::vector<float> correct(float drift, float vibrato, std::span<const double> shift = {}, std::span<const Marker> markers = {},
                             std::span<const mx_formant_point> points = {}, int glideFrames = 8) const;

private:
  int sampleRate, hop_, device_;
  bool good = false;
  std::vector<float> wav_;
  std::vector<mx_f0> track;
  std::vector<mx_note> notes_;
  std::vector<mx_contour_span> spans;
  std::vector<mx_contour_rec> rec;
  std::vector<mx_contour_stat> stat;
  std::vector<mx_vibrato> vibrato_;
};

}  // namespace melonix
