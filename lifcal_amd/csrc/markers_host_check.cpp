// markers_host_check.cpp — the host-only part of include/lifcal_markers.h (markers_host.hpp) as a stand-alone program, so that the
// argument checks, the dictionary code, the quad, the constraints reader, the start values and the scale factor can run under the
// host sanitizers:
//   make -C lifcal_amd/csrc markers_host_check && lifcal_amd/csrc/markers_host_check
// (the target compiles with -fsanitize=address,undefined).  No HIP, no device, no Python.  Every array is allocated at its exact
// size so that a read or write past an end is caught; the constraints files are written to the working directory and removed.
#include <cstdio>
#include <cstring>

#include "markers_host.hpp"

namespace lifcal {
static std::string g_error;
void set_last_error(const char* text) { g_error = text; }
}  // namespace lifcal

using namespace lifcal::markers;

static int g_failed = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
  } while (0)

static bool said(const char* word) { return lifcal::g_error.find(word) != std::string::npos; }

struct Read {
  int rc = 0;
  std::vector<uint32_t> a, b, ids;
  std::vector<double> dist, sig;
};

// count, then fill, with exactly-sized heap arrays
static Read read_file(const char* text) {
  const char* path = "markers_host_check.tmp";
  Read r;
  if (text) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) { r.rc = -100; return r; }
    std::fwrite(text, 1, std::strlen(text), f);
    std::fclose(f);
  }
  lifcal_constraints io{};
  r.rc = read_constraints(text ? path : "markers_host_check.missing", &io);
  if (r.rc == LIFCAL_MLA_MORE) {
    r.a.resize(io.n); r.b.resize(io.n); r.dist.resize(io.n); r.sig.resize(io.n); r.ids.resize(io.n_ids);
    io.capacity = io.n; io.ids_capacity = io.n_ids;
    io.id1 = r.a.data(); io.id2 = r.b.data(); io.distance = r.dist.data(); io.sigma = r.sig.data(); io.ids = r.ids.data();
    r.rc = read_constraints(path, &io);
  }
  if (text) std::remove(path);
  return r;
}

int main() {
  using U = std::vector<uint32_t>;
  {  // words, rotations, distances
    const uint64_t w = 0x1234;
    EXPECT(rot_word(rot_word(rot_word(rot_word(w, 4), 4), 4), 4) == w && rot_word(w, 4) != w);
    EXPECT(rot_word(1ull, 3) == (1ull << 2) && rot_word(1ull << 2, 3) == (1ull << 8));   // top-left -> top-right -> bottom-right
    EXPECT(word_distance(w, rot_word(w, 4), 4, 0) == 0 && word_distance(w, w, 4, 1) > 0);
    const std::vector<uint64_t> sym{0x10};   // the centre of a 3 x 3 grid: its own rotation
    lifcal_marker_dictionary d{3, 1, sym.data()};
    EXPECT(check_dictionary("t: ", &d) == 0 && dictionary_distance(&d) == 0);
    const std::vector<uint64_t> high{1ull << 9};
    d.words = high.data();
    EXPECT(check_dictionary("t: ", &d) == LIFCAL_BA_ERR_INVALID_ARG && said("above"));
    d.marker_bits = 8;
    EXPECT(check_dictionary("t: ", &d) == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(check_dictionary("t: ", nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
  }
  {  // the generator: deterministic, exact size, every word apart from the others and from its own rotations
    for (int bits = 3; bits <= 7; ++bits) {
      const uint32_t n = bits == 3 ? 10 : 50;
      std::vector<uint64_t> a(n), b(n);
      int32_t da = -1, db = -1;
      EXPECT(generate_dictionary(bits, n, 1, a.data(), &da) == 0 && generate_dictionary(bits, n, 1, b.data(), &db) == 0);
      EXPECT(a == b && da == db && da >= 1);
      for (uint64_t v : a) EXPECT((v >> (bits * bits)) == 0);
      EXPECT(generate_dictionary(bits, n, 2, b.data(), nullptr) == 0 && a != b);
    }
    std::vector<uint64_t> out(400);
    EXPECT(generate_dictionary(3, 400, 1, out.data(), nullptr) == LIFCAL_BA_ERR_OUT_OF_RANGE);
    EXPECT(generate_dictionary(2, 4, 1, out.data(), nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(generate_dictionary(4, 0, 1, out.data(), nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(generate_dictionary(4, 4, 1, nullptr, nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
  }
  {  // the plan and its refusals
    uint16_t px[4] = {0, 0, 0, 0};
    lifcal_rawdepth_image im{px, 8, 203, 131, 0, 203};
    std::vector<uint64_t> words(50);
    int32_t dmin = 0;
    EXPECT(generate_dictionary(4, 50, 1, words.data(), &dmin) == 0);
    lifcal_marker_dictionary d{4, 50, words.data()};
    Plan t;
    EXPECT(make_plan("check", &im, &d, nullptr, &t) == 0 && t.opt.w == 7 && t.opt.cell_contrast == 24 && t.opt.max_side == 131 && t.tx == 7 && t.ty == 5);
    EXPECT(t.min_distance == dmin && t.opt.max_correction == (dmin - 1) / 2 && t.max_candidates == 203 * 131 / 32 && t.C == 12 && t.C_cell == 24);
    im.bits = 16;
    EXPECT(make_plan("check", &im, &d, nullptr, &t) == 0 && t.C == 12 * 256);
    lifcal_markers_options o{};
    o.max_correction = (dmin - 1) / 2 + 1;
    EXPECT(make_plan("check", &im, &d, &o, &t) == LIFCAL_BA_ERR_INVALID_ARG && said("max_correction"));
    o.max_correction = -1;
    EXPECT(make_plan("check", &im, &d, &o, &t) == 0 && t.opt.max_correction == 0);
    o = lifcal_markers_options{}; o.w = 32;
    EXPECT(make_plan("check", &im, &d, &o, &t) == LIFCAL_BA_ERR_INVALID_ARG && said("w outside"));
    o = lifcal_markers_options{}; o.refine_max = -1.0;
    EXPECT(make_plan("check", &im, &d, &o, &t) == LIFCAL_BA_ERR_INVALID_ARG);
    o = lifcal_markers_options{}; o.max_border_errors = 21;
    EXPECT(make_plan("check", &im, &d, &o, &t) == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(make_plan("check", &im, nullptr, &o, &t) == 0);   // without a dictionary the bound is that of 7 bits
    im.pitch = 202;
    EXPECT(make_plan("check", &im, &d, nullptr, &t) == LIFCAL_BA_ERR_INVALID_ARG && said("pitch"));
    im.pitch = im.width = 1 << 16; im.height = 1 << 15;
    EXPECT(make_plan("check", &im, &d, nullptr, &t) == LIFCAL_BA_ERR_OUT_OF_RANGE);
    EXPECT(make_plan("check", nullptr, &d, nullptr, &t) == LIFCAL_BA_ERR_INVALID_ARG);
  }
  {  // candidates and the quad
    lifcal_markers_options o{};
    o.min_area = 32; o.min_side = 12; o.max_side = 100;
    lifcal_marker_component c{};
    const int32_t sq[8][2] = {{10, 10}, {30, 10}, {10, 10}, {10, 30}, {10, 10}, {30, 30}, {10, 30}, {30, 10}};
    std::memcpy(c.ext, sq, sizeof(sq));
    c.area = 80;
    EXPECT(is_candidate(&c, o, 64, 64) && c.x0 == 10 && c.x1 == 30 && c.y0 == 10 && c.y1 == 30);
    EXPECT(!is_candidate(&c, o, 31, 64) && !is_candidate(&c, o, 64, 31));   // the box touches the right or the lower border
    c.area = 31;
    EXPECT(!is_candidate(&c, o, 64, 64));
    std::vector<double> q(8);
    EXPECT(choose_quad(&c.ext[0][0], 12, q.data()) && q[0] == 9.5 && q[1] == 9.5 && q[2] == 30.5 && q[3] == 9.5 && q[4] == 30.5 && q[5] == 30.5 && q[6] == 9.5 &&
           q[7] == 30.5);
    EXPECT(choose_quad(&c.ext[0][0], 28, q.data()) && !choose_quad(&c.ext[0][0], 29, q.data()));   // 2 * 20 * 20 against min_side^2
    const int32_t di[8][2] = {{0, 20}, {40, 20}, {20, 0}, {20, 40}, {20, 0}, {20, 40}, {0, 20}, {40, 20}};   // a diamond: the axis set
    EXPECT(choose_quad(&di[0][0], 12, q.data()) && q[0] == 20.0 && q[1] == -0.5 && q[2] == 40.5 && q[3] == 20.0 && q[6] == -0.5 && q[7] == 20.0);
    // both sets of double area 576: the diagonal set wins
    const int32_t tie[8][2] = {{20, 32}, {44, 32}, {32, 20}, {32, 44}, {24, 23}, {40, 41}, {24, 41}, {40, 23}};
    EXPECT(choose_quad(&tie[0][0], 12, q.data()) && q[0] == 23.5 && q[1] == 22.5 && q[2] == 40.5 && q[3] == 22.5 && q[4] == 40.5 && q[5] == 41.5);
  }
  {  // the constraints reader
    Read r = read_file("# id1 id2 distance sigma\n\n7 3 0.25 0.001\n3 12 1.5e-1 2e-3\r\n#7 7 1 1\n 12 7 0.3 0.01  \n\n");
    EXPECT(r.rc == 0 && (r.a == U{7, 3, 12}) && (r.b == U{3, 12, 7}) && (r.ids == U{7, 3, 12}));
    EXPECT(r.dist.size() == 3 && r.dist[1] == 0.15 && r.sig[2] == 0.01);
    r = read_file("# nothing\n\n");
    EXPECT(r.rc == 0 && r.a.empty() && r.ids.empty());
    r = read_file("1 2 0.5 0.1");   // no newline at the end
    EXPECT(r.rc == 0 && r.a.size() == 1);
    const char* bad[] = {"1 2 0.5\n", "1 x 0.5 0.1\n", "1 2 0.5 0.1 9\n", "-1 2 0.5 0.1\n", "1 2 -0.5 0.1\n", "1 2 0.5 0\n", "1 2 nan 0.1\n", "1.5 2 0.5 0.1\n", "   \n",
                         "99999999999999999999 2 0.5 0.1\n", "1 2 1e999 0.1\n"};
    for (const char* text : bad) EXPECT(read_file(text).rc == LIFCAL_BA_ERR_INVALID_ARG && said("line 1"));
    EXPECT(read_file(nullptr).rc == LIFCAL_BA_ERR_INVALID_ARG && said("cannot open"));
    EXPECT(read_constraints(nullptr, nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
  }
  {  // start values: ties, the first frame, a frame without tracked points, indices out of range
    const std::vector<double> mx{20, 50.4, 70, 5, 6}, my{20, 50, 70, 5, 6};
    const U mfr{0, 1, 1, 2, 2}, mid{4, 9, 4, 9, 1};
    const std::vector<double> tx{10, 30, 20, 20, 50, 51, 70}, ty{20, 20, 10, 30, 50, 50, 70};
    const U tfr{0, 0, 0, 0, 1, 1, 1}, tpt{2, 3, 4, 5, 0, 1, 2};
    std::vector<double> pts(18);
    for (size_t i = 0; i < pts.size(); ++i) pts[i] = 0.5 * (double)i;
    lifcal_marker_seeds io{};
    EXPECT(seed_points(5, mx.data(), my.data(), mfr.data(), mid.data(), 7, tx.data(), ty.data(), tfr.data(), tpt.data(), 6, pts.data(), &io) == LIFCAL_MLA_MORE);
    EXPECT(io.n_ids == 3 && io.n_unseeded == 1);
    U ids(3);
    std::vector<double> xyz(9);
    std::vector<uint8_t> seeded(3);
    io.capacity = 3; io.ids = ids.data(); io.xyz = xyz.data(); io.seeded = seeded.data();
    EXPECT(seed_points(5, mx.data(), my.data(), mfr.data(), mid.data(), 7, tx.data(), ty.data(), tfr.data(), tpt.data(), 6, pts.data(), &io) == 0);
    EXPECT((ids == U{4, 9, 1}) && seeded[0] == 1 && seeded[1] == 1 && seeded[2] == 0);
    EXPECT(xyz[0] == pts[6] && xyz[2] == pts[8] && xyz[3] == pts[0] && xyz[8] == 0.0);   // point 2 (the first of four at equal distance), point 0
    EXPECT(seed_points(5, mx.data(), my.data(), mfr.data(), mid.data(), 7, tx.data(), ty.data(), tfr.data(), tpt.data(), 5, pts.data(), &io) ==
           LIFCAL_BA_ERR_OUT_OF_RANGE);
    EXPECT(seed_points(0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &io) == 0 && io.n_ids == 0);
    EXPECT(seed_points(5, mx.data(), nullptr, mfr.data(), mid.data(), 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &io) == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(seed_points(0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
  }
  {  // the scale factor
    const double p1[3] = {0.1, -0.2, 3.0}, p2[3] = {0.4, 0.2, 3.0}, bad[3] = {0.0, std::nan(""), 0.0};
    double f = 0.0;
    EXPECT(scale_factor(p1, p2, 0.25, &f) == 0 && std::fabs(f - 0.5) < 1e-15);
    EXPECT(scale_factor(p1, p1, 0.25, &f) == LIFCAL_BA_ERR_NUMERIC && scale_factor(p1, bad, 0.25, &f) == LIFCAL_BA_ERR_NUMERIC);
    EXPECT(scale_factor(p1, p2, 0.0, &f) == LIFCAL_BA_ERR_INVALID_ARG && scale_factor(p1, p2, -1.0, &f) == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(scale_factor(nullptr, p2, 0.25, &f) == LIFCAL_BA_ERR_INVALID_ARG && scale_factor(p1, p2, 0.25, nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
  }
  std::printf(g_failed ? "markers_host_check: %d FAILED\n" : "markers_host_check ok\n", g_failed);
  return g_failed ? 1 : 0;
}
