// Stand-alone driver of the host side of cy_forced_fit (caesar_yolo_amd/csrc/cy_measure_plan.cpp) for tests/test_forced_plan_cpu.py,
// which builds it with the host sanitizers: no HIP, no GPU library.  It does what the entry does around its launch: plan_forced,
// a table of one row per run job in place of the kernel's, and forced_row for every job.
//
//     forced_plan_main MH MW N NSIGMA FIT_BKG NULLS [COLS] < numbers
// NULLS: a string of the letters m, j, o naming the pointers that are passed as null ("-": none).  Without COLS, standard input holds N
// jobs of six numbers (x0 y0 a b c bkg), as C99 hexadecimal floats or "nan" / "inf" / "-inf"; with a negative or oversize N nothing
// is read.  With COLS nothing is read and job i is made here: a lattice of COLS columns, 5 pixels between neighbours in a row and 6
// between rows, x0 = 5 (i % COLS) + 0.25, y0 = 6 (i / COLS) + 0.5, a = c = 4 (sigma 0.5), b = 0, bkg = i; every 7th job has a = 0
// (status 1) and every 11th a centre of 1e300 (status 3).
// The stand-in for the kernel's row t (the t-th run job) holds 1000 t + f + 0.5 in field f.
// Prints "error <message>", or "ok <run jobs>" and then
//     without COLS  two lines per job: the CY_FORCED_FIELDS numbers of its row as hexadecimal floats, and "n" followed by its kept
//                   neighbours
//     with COLS     "counts <run> <status 1> <status 3>", "sums <nneigh> <widths> <heights> <crowded> <ndup>" over the run rows, the
//                   number of fields that are not what the stand-in (or the turned-away rule) says, and the rows of jobs 0, 1,
//                   COLS and N - 1
#include "../../caesar_yolo_amd/csrc/cy_measure_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace cy;

static bool number(double* v) {
    char tok[128];
    if (std::scanf("%127s", tok) != 1) return false;
    *v = std::strtod(tok, nullptr);
    return true;
}

static void print_row(const double* r) {
    for (int f = 0; f < FORCED_FIELDS; ++f) std::printf(f ? " %a" : "%a", r[f]);
    std::printf("\n");
}

static bool plan_field(int f) { return (f >= 3 && f <= 6) || (f >= 17 && f <= 21); }

int main(int argc, char** argv) {
    if (argc != 7 && argc != 8) { std::fprintf(stderr, "usage: forced_plan_main MH MW N NSIGMA FIT_BKG NULLS [COLS]\n"); return 2; }
    const int MH = (int)std::strtol(argv[1], nullptr, 10), MW = (int)std::strtol(argv[2], nullptr, 10), n = (int)std::strtol(argv[3], nullptr, 10);
    const double nsigma = std::strtod(argv[4], nullptr);
    const int fit_bkg = (int)std::strtol(argv[5], nullptr, 10);
    const char* nulls = argv[6];
    const int cols = argc == 8 ? (int)std::strtol(argv[7], nullptr, 10) : 0;
    const bool in_range = n >= 0 && n <= FORCED_JOBS_MAX;
    std::vector<double> jobs(in_range ? (size_t)n * FORCED_JOB_FIELDS : 0);     // exactly sized: a read past n jobs is a sanitizer report
    if (cols > 0) {
        for (int i = 0; in_range && i < n; ++i) {
            double* q = &jobs[(size_t)i * FORCED_JOB_FIELDS];
            q[0] = 5.0 * (i % cols) + 0.25; q[1] = 6.0 * (i / cols) + 0.5; q[2] = i % 7 == 6 ? 0.0 : 4.0; q[3] = 0.0; q[4] = 4.0; q[5] = (double)i;
            if (i % 11 == 10) q[0] = 1e300;
        }
    } else {
        for (double& j : jobs) if (!number(&j)) { std::fprintf(stderr, "short input\n"); return 2; }
    }
    ForcedPlan p;
    const char* msg = plan_forced(std::strchr(nulls, 'j') ? nullptr : jobs.data(), n, nsigma, fit_bkg, MH, MW, !std::strchr(nulls, 'm'), !std::strchr(nulls, 'o'), p);
    if (msg) { std::printf("error %s\n", msg); return 0; }
    if ((long long)p.jobs.size() != n) { std::fprintf(stderr, "%zu jobs planned for n = %d\n", p.jobs.size(), n); return 3; }
    // what the entry does after its launch, with exactly sized buffers
    std::vector<double> got(p.run.size() * FORCED_FIELDS), out((size_t)n * FORCED_FIELDS);
    for (size_t t = 0; t < p.run.size(); ++t)
        for (int f = 0; f < FORCED_FIELDS; ++f) got[t * FORCED_FIELDS + f] = 1000.0 * (double)t + f + 0.5;
    size_t next = 0;
    for (int i = 0; i < n; ++i) {
        const bool ran = next < p.run.size() && p.run[next] == i;
        forced_row(p.jobs[(size_t)i], fit_bkg, ran ? &got[next * FORCED_FIELDS] : nullptr, &out[(size_t)i * FORCED_FIELDS]);
        next += ran;
    }
    if (next != p.run.size()) { std::fprintf(stderr, "%zu of %zu rows dealt out\n", next, p.run.size()); return 3; }
    std::printf("ok %zu\n", p.run.size());
    if (cols <= 0) {
        for (int i = 0; i < n; ++i) {
            print_row(&out[(size_t)i * FORCED_FIELDS]);
            std::printf("n");
            for (int k = 0; k < p.jobs[(size_t)i].nneigh; ++k) std::printf(" %d", p.jobs[(size_t)i].neigh[k]);
            std::printf("\n");
        }
        return 0;
    }
    long long cnt[3] = {0, 0, 0}, nneigh = 0, w = 0, h = 0, crowded = 0, ndup = 0, wrong = 0;
    size_t t = 0;
    for (int i = 0; i < n; ++i) {
        const double* r = &out[(size_t)i * FORCED_FIELDS];
        const ForcedJob& j = p.jobs[(size_t)i];
        if (j.status == 0 || j.status == 2) {
            ++cnt[0];
            for (int f = 0; f < FORCED_FIELDS; ++f)
                if (!plan_field(f)) wrong += r[f] != 1000.0 * (double)t + f + 0.5;
            nneigh += (long long)r[4]; w += (long long)(r[18] - r[17] + 1.0); h += (long long)(r[20] - r[19] + 1.0); crowded += (long long)r[5];
            ndup += (long long)r[6];
            wrong += r[3] != 1.0 + r[4] + fit_bkg;
            ++t;
        } else {
            ++cnt[j.status == 1 ? 1 : 2];
            for (int f = 0; f < FORCED_FIELDS; ++f) {
                const double want = f == 0 ? (double)j.status : (f >= 17 && f <= 20) ? -1.0 : 0.0;
                wrong += r[f] != want;
            }
        }
    }
    std::printf("counts %lld %lld %lld\nsums %lld %lld %lld %lld %lld\nwrong %lld\n", cnt[0], cnt[1], cnt[2], nneigh, w, h, crowded, ndup, wrong);
    const int show[4] = {0, 1, cols, n - 1};
    for (int k = 0; k < 4; ++k)
        if (show[k] >= 0 && show[k] < n) print_row(&out[(size_t)show[k] * FORCED_FIELDS]);
    return 0;
}
