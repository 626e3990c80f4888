// driver_common.hpp — what the small facade drivers of tests/cpp share: the GL calls the headless facade (NO_GL) leaves to the
// embedding program, as no-ops (these programs make no texture; facade_driver.cpp and facade_stress.cpp count theirs and keep
// their own), and raw files in and out.
#pragma once
#include <cstdio>
#include <vector>

#include "gl_sink.hpp"

extern "C" {
void glGenTextures(GLsizei, GLuint *) {}
void glDeleteTextures(GLsizei, const GLuint *) {}
void glBindTexture(GLenum, GLuint) {}
void glTexParameteri(GLenum, GLenum, GLint) {}
void glTexImage1D(GLenum, GLint, GLint, GLsizei, GLint, GLenum, GLenum, const void *) {}
}

// the raw float32 samples of a file; false: it does not open
static bool read_f32(const char *path, std::vector<float> &wav) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  float buf[4096];
  size_t k;
  while ((k = std::fread(buf, sizeof(float), 4096, f)) > 0) wav.insert(wav.end(), buf, buf + k);
  std::fclose(f);
  return true;
}

// the records of v, raw, as a file; false: not all of them got there
template <class T>
static bool dump(const char *path, const std::vector<T> &v) {
  FILE *o = std::fopen(path, "wb");
  if (!o) return false;
  const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), o) == v.size();
  return std::fclose(o) == 0 && ok;
}
