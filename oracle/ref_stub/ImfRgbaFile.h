/*
 * Stand-in for OpenEXR's <ImfRgbaFile.h>, written for this project: the few names the reference's feature-image writer
 * and image reader mention, so that those files compile where OpenEXR is absent.  Nothing is read or written: the output
 * file accepts its pixels and drops them, the input file refuses to open.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/Makefile target `ref_full`).
 */
#ifndef RPF_ORACLE_IMF_STAND_IN_H
#define RPF_ORACLE_IMF_STAND_IN_H

/* the reference's visualization header leans on these arriving with the OpenEXR headers */
#include <algorithm>
#include <cstddef>
#include <stdexcept>
#include <string>

namespace Imath {
struct V2i {
    int x, y;
    V2i() : x(0), y(0) {}
    V2i(int x_, int y_) : x(x_), y(y_) {}
};
struct Box2i {
    V2i min, max;
    Box2i() {}
    Box2i(const V2i &lo, const V2i &hi) : min(lo), max(hi) {}
};
}  // namespace Imath

namespace Imf {

struct Rgba {
    float r, g, b, a;
    Rgba() : r(0), g(0), b(0), a(0) {}
    Rgba(float r_, float g_, float b_, float a_ = 1.f) : r(r_), g(g_), b(b_), a(a_) {}
};

enum RgbaChannels { WRITE_RGB = 7, WRITE_RGBA = 15 };

class RgbaOutputFile {
  public:
    RgbaOutputFile(const char *, int, int, RgbaChannels = WRITE_RGBA) {}
    RgbaOutputFile(const char *, const Imath::Box2i &, const Imath::Box2i &, RgbaChannels = WRITE_RGBA) {}
    void setFrameBuffer(const Rgba *, size_t, size_t) {}
    void writePixels(int = 1) {}
};

class RgbaInputFile {
  public:
    explicit RgbaInputFile(const char *name) { throw std::runtime_error(std::string("no OpenEXR here: ") + name); }
    const Imath::Box2i &dataWindow() const { return window_; }
    const Imath::Box2i &displayWindow() const { return window_; }
    void setFrameBuffer(Rgba *, size_t, size_t) {}
    void readPixels(int, int) {}

  private:
    Imath::Box2i window_;
};

}  // namespace Imf

#endif  // RPF_ORACLE_IMF_STAND_IN_H
