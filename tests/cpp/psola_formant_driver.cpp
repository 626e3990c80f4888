// psola_formant_driver.cpp — the melonix::Resynth::renderPSOLA / exportWavPSOLA overloads that take formant points, from a
// compiled program (tests/test_gpu_psola_formant_facade.py):
//   psola_formant_driver <in.f32> <sampleRate> <bend> <formant0> <formant1> <out.f32> <out.wav>
// reads raw float32 samples, tracks them, renders them retuned by a constant <bend> semitones with the envelope moved along
// a ramp from <formant0> at sample 0 to <formant1> at the last sample, writes the float PCM raw and the int16 PCM through
// saveWav.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gl_sink.hpp"
#include "melonix_amd.h"
#include "pitch-track.hpp"
#include "resynth.hpp"

// the headless facade (NO_GL) leaves its few GL calls to the embedding program; this one makes no texture
extern "C" {
void glGenTextures(GLsizei, GLuint *) {}
void glDeleteTextures(GLsizei, const GLuint *) {}
void glBindTexture(GLenum, GLuint) {}
void glTexParameteri(GLenum, GLenum, GLint) {}
void glTexImage1D(GLenum, GLint, GLint, GLsizei, GLint, GLenum, GLenum, const void *) {}
}

int main(int argc, char **argv) {
  if (argc != 8) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<float> wav;
  float buf[4096];
  size_t k;
  while ((k = std::fread(buf, sizeof(float), 4096, f)) > 0) wav.insert(wav.end(), buf, buf + k);
  std::fclose(f);
  const int sr = std::atoi(argv[2]);
  const double bend = std::atof(argv[3]);
  melonix::PitchTrack track(wav, sr, 256);
  if (!track.ok()) return 4;
  melonix::Resynth rs(wav, sr);
  if (!rs.ok()) return 5;
  const std::vector<Marker> mk = {{1, 0, 0, bend}, {(int)wav.size() - 1, 0, 0, bend}};
  const std::vector<mx_formant_point> pts = {{0, (float)std::atof(argv[4])}, {(int32_t)wav.size() - 1, (float)std::atof(argv[5])}};
  const std::vector<float> pcm = rs.renderPSOLA(mk, track.frames(), track.hop(), pts);
  if (pcm.empty()) return 6;
  FILE *o = std::fopen(argv[6], "wb");
  if (!o) return 7;
  std::fwrite(pcm.data(), sizeof(float), pcm.size(), o);
  std::fclose(o);
  if (!rs.exportWavPSOLA(argv[7], mk, track.frames(), track.hop(), pts)) return 8;
  // no points: the plain overload's samples
  if (rs.renderPSOLA(mk, track.frames(), track.hop(), std::vector<mx_formant_point>()) != rs.renderPSOLA(mk, track.frames(), track.hop()))
    return 9;
  // a curve whose samples do not increase is refused: an empty vector, no file
  const std::vector<mx_formant_point> bad = {{100, 1.f}, {100, 2.f}};
  if (!rs.renderPSOLA(mk, track.frames(), track.hop(), bad).empty()) return 10;
  std::printf("%zu frames, %zu samples, %zu points\n", track.frames().size(), pcm.size(), pts.size());
  return 0;
}
