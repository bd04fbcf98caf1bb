// Stand-alone driver of the measurement planner (caesar_yolo_amd/csrc/cy_measure_plan.cpp) for tests/test_measure_plan_cpu.py,
// which builds it with the host sanitizers: no HIP, no GPU library.
//
//     measure_plan_main {sources|islands|deblend|fit|blend} CASE OUT
//
// CASE: int32 {MH, MW, n, ring, has_off}, then seven blobs (int64 byte count + bytes): boxes f64 [n][4], thr f64 [n][3 or 4],
// ncomp i32 [n], bkg f64 [n], start f64 [n][16][6], mask_off i64 [n + 1], mask u8.  A blob the mode does not read may be empty.
// OUT: int32 0 and the planner's outputs as blobs (the job records field by field), or int32 1 and the error message.  The fit
// modes end with the rows the entry would return had the device answered with fake_table(): write_back() over every job.
#include "../../caesar_yolo_amd/csrc/cy_measure_plan.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace cy;

namespace {
[[noreturn]] void die(const char* what) { std::fprintf(stderr, "measure_plan_main: %s\n", what); std::exit(2); }

std::vector<char> read_file(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) die("cannot open the case file");
    std::vector<char> buf;
    char chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(f);
    return buf;
}

struct Case {
    std::vector<char> buf; size_t pos = 0;
    int32_t hdr[5];
    // a blob as an array of T with exactly `count` elements (copied: the planner gets aligned, exactly sized arrays)
    template <class T> std::vector<T> blob(size_t count, bool wanted) {
        int64_t bytes;
        if (pos + sizeof(bytes) > buf.size()) die("truncated case file");
        std::memcpy(&bytes, &buf[pos], sizeof(bytes)); pos += sizeof(bytes);
        if (bytes < 0 || (size_t)bytes > buf.size() - pos) die("truncated blob");
        std::vector<T> v;
        if (wanted) {
            if ((size_t)bytes != count * sizeof(T)) die("a blob has the wrong size for this mode");
            v.resize(count);
            if (bytes) std::memcpy(v.data(), &buf[pos], (size_t)bytes);
        }
        pos += (size_t)bytes;
        return v;
    }
};

struct Out {
    FILE* f;
    void i32(int32_t v) { std::fwrite(&v, sizeof(v), 1, f); }
    template <class T> void blob(const std::vector<T>& v) {
        const int64_t bytes = (int64_t)(v.size() * sizeof(T));
        std::fwrite(&bytes, sizeof(bytes), 1, f);
        if (bytes) std::fwrite(v.data(), 1, (size_t)bytes, f);
    }
    // one field of every job, `len` values each
    template <class T, class Job, class Get> void field(const std::vector<Job>& jobs, int len, Get get) {
        std::vector<T> v;
        for (const Job& j : jobs) for (int t = 0; t < len; ++t) v.push_back(get(j, t));
        blob(v);
    }
    void error(const char* msg) { i32(1); std::fwrite(msg, 1, std::strlen(msg), f); }
};

// a device table [nrows][width] to write back: status r % 5 (3 and 4: not fitted), field f of row r = 1000 r + f
std::vector<double> fake_table(size_t nrows, int width) {
    std::vector<double> v(nrows * width);
    for (size_t r = 0; r < nrows; ++r) {
        for (int f = 1; f < width; ++f) v[r * width + f] = 1000.0 * (double)r + f;
        v[r * width] = (double)(r % 5);
    }
    return v;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) die("usage: measure_plan_main {sources|islands|deblend|fit|blend} CASE OUT");
    const std::string mode = argv[1];
    const bool isl = mode == "islands" || mode == "deblend", fit = mode == "fit" || mode == "blend";
    if (mode != "sources" && !isl && !fit) die("unknown mode");
    Case c;
    c.buf = read_file(argv[2]);
    if (c.buf.size() < sizeof(c.hdr)) die("truncated case file");
    std::memcpy(c.hdr, c.buf.data(), sizeof(c.hdr)); c.pos = sizeof(c.hdr);
    const int MH = c.hdr[0], MW = c.hdr[1], n = c.hdr[2], ring = c.hdr[3];
    const bool has_off = c.hdr[4] != 0;
    if (MH <= 0 || MW <= 0 || n <= 0 || ring < 0 || (long long)MH * MW >= (1LL << 31)) die("the entries reject this header before they plan");
    const int stride = mode == "deblend" ? 4 : 3;
    const auto boxes = c.blob<double>((size_t)n * 4, true);
    const auto thr = c.blob<double>((size_t)n * stride, isl);
    const auto ncomp = c.blob<int32_t>((size_t)n, fit);
    const auto bkg = c.blob<double>((size_t)n, fit);
    const auto start = c.blob<double>((size_t)n * DBL_MAX_COMP * 6, fit);
    const auto mask_off = c.blob<long long>((size_t)n + 1, fit || (isl && has_off));
    // the mask of the fit modes: as many bytes as the last offset claims (the planner checks the offsets before it reads a byte
    // of a source, so a wrong table is rejected within the bytes of the windows before it)
    int64_t mask_bytes = 0;
    if (fit) {
        if (c.pos + 8 > c.buf.size()) die("truncated case file");
        std::memcpy(&mask_bytes, &c.buf[c.pos], 8);
    }
    const auto mask = c.blob<unsigned char>((size_t)mask_bytes, fit);

    Out o{std::fopen(argv[3], "wb")};
    if (!o.f) die("cannot open the output file");
    if (mode == "sources") {
        o.i32(0);
        o.blob(ring_windows(boxes.data(), n, ring, MH, MW));
    } else if (isl) {
        IslandTable t;
        if (const char* msg = plan_islands(boxes.data(), thr.data(), stride, has_off ? mask_off.data() : nullptr, n, MH, MW, t)) o.error(msg);
        else {
            o.i32(0);
            o.blob(t.win); o.blob(t.off); o.blob(std::vector<long long>{t.nws, t.nmask});
        }
    } else {
        const unsigned char none = 0;                          // the entries want a mask pointer even when every window is empty
        const FitInputs in{MH, MW, n, boxes.data(), bkg.data(), ncomp.data(), start.data(), mask.empty() ? &none : mask.data(), mask_off.data()};
        if (mode == "fit") {
            FitPlan p;
            if (const char* msg = plan_fit(in, p)) o.error(msg);
            else {
                o.i32(0);
                o.field<long long>(p.jobs, 1, [](const FitJob& j, int) { return j.list_off; });
                o.field<unsigned>(p.jobs, 1, [](const FitJob& j, int) { return j.npos; });
                o.field<int>(p.jobs, 1, [](const FitJob& j, int) { return j.x0; });
                o.field<int>(p.jobs, 1, [](const FitJob& j, int) { return j.y0; });
                o.field<unsigned>(p.jobs, 1, [](const FitJob& j, int) { return j.W; });
                o.field<unsigned>(p.jobs, 1, [](const FitJob& j, int) { return j.A; });
                o.field<int>(p.jobs, 1, [](const FitJob& j, int) { return j.row; });
                o.field<double>(p.jobs, 1, [](const FitJob& j, int) { return j.bkg; });
                o.field<double>(p.jobs, 6, [](const FitJob& j, int t) { return j.p0[t]; });
                o.blob(p.list); o.blob(p.win0); o.blob(p.large);
                const size_t nrows = (size_t)n * DBL_MAX_COMP;
                const std::vector<double> got = fake_table(nrows, FIT_FIELDS);
                std::vector<double> back(got.size(), 0.0);
                for (const FitJob& j : p.jobs) write_back(got.data(), start.data(), p.win0.data(), FIT_FIELDS, 5, &j.row, 1, back.data());
                o.blob(back);
            }
        } else {
            BlendPlan p;
            if (const char* msg = plan_blend(in, p)) o.error(msg);
            else {
                o.i32(0);
                o.field<long long>(p.jobs, 1, [](const BlendJob& j, int) { return j.list_off; });
                o.field<unsigned>(p.jobs, 1, [](const BlendJob& j, int) { return j.npos; });
                o.field<int>(p.jobs, 1, [](const BlendJob& j, int) { return j.x0; });
                o.field<int>(p.jobs, 1, [](const BlendJob& j, int) { return j.y0; });
                o.field<unsigned>(p.jobs, 1, [](const BlendJob& j, int) { return j.W; });
                o.field<unsigned>(p.jobs, 1, [](const BlendJob& j, int) { return j.A; });
                o.field<int>(p.jobs, 1, [](const BlendJob& j, int) { return j.row0; });
                o.field<int>(p.jobs, 1, [](const BlendJob& j, int) { return j.M; });
                o.field<int>(p.jobs, BLEND_MAX_MEMBERS, [](const BlendJob& j, int t) { return j.comp[t]; });
                o.field<double>(p.jobs, 1, [](const BlendJob& j, int) { return j.bkg; });
                o.field<double>(p.jobs, 6 * BLEND_MAX_MEMBERS, [](const BlendJob& j, int t) { return j.p0[t]; });
                o.blob(p.list); o.blob(p.win0); o.blob(p.rows);
                const std::vector<double> got = fake_table((size_t)n * DBL_MAX_COMP, BLEND_FIELDS);
                std::vector<double> back = p.rows;
                for (const BlendJob& j : p.jobs) {
                    int rows[BLEND_MAX_MEMBERS];
                    for (int m = 0; m < j.M; ++m) rows[m] = j.row0 + j.comp[m];
                    write_back(got.data(), start.data(), p.win0.data(), BLEND_FIELDS, 8, rows, j.M, back.data());
                }
                o.blob(back);
            }
        }
    }
    if (std::fclose(o.f) != 0) die("cannot write the output file");
    return 0;
}
