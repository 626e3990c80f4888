// psola_driver.cpp — melonix::PitchTrack + melonix::Resynth::renderPSOLA / exportWavPSOLA from a compiled program
// (tests/test_gpu_psola_facade.py):
//   psola_driver <in.f32> <sampleRate> <bend> <decoded 0|1> <out.f32> <out.wav>
// reads raw float32 samples, tracks them, renders them retuned by a constant <bend> semitones with the track's own voicing
// parameters, writes the float PCM raw and the int16 PCM through saveWav.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gl_sink.hpp"
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
  if (argc != 7) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<float> wav;
  float buf[4096];
  size_t k;
  while ((k = std::fread(buf, sizeof(float), 4096, f)) > 0) wav.insert(wav.end(), buf, buf + k);
  std::fclose(f);
  const int sr = std::atoi(argv[2]);
  const double bend = std::atof(argv[3]);
  melonix::PitchTrack track(wav, sr, 256, 55.f, 1760.f, 0.15f, 0, std::atoi(argv[4]) != 0);
  if (!track.ok()) return 4;
  melonix::Resynth rs(wav, sr);
  if (!rs.ok()) return 5;
  const std::vector<Marker> mk = {{1, 0, 0, bend}, {(int)wav.size() - 1, 0, 0, bend}};
  const mx_psola_params p = track.psolaParams();
  const std::vector<float> pcm = rs.renderPSOLA(mk, track.frames(), track.hop(), &p);
  if (pcm.empty()) return 6;
  FILE *o = std::fopen(argv[5], "wb");
  if (!o) return 7;
  std::fwrite(pcm.data(), sizeof(float), pcm.size(), o);
  std::fclose(o);
  if (!rs.exportWavPSOLA(argv[6], mk, track.frames(), track.hop(), &p)) return 8;
  // a track that does not fit the file is refused: an empty vector, no file
  std::vector<mx_f0> shortTrack(track.frames().begin(), track.frames().end() - 1);
  if (!rs.renderPSOLA(mk, shortTrack, track.hop()).empty()) return 9;
  std::printf("%zu frames, %zu samples, threshold %g\n", track.frames().size(), pcm.size(), (double)p.threshold);
  return 0;
}
