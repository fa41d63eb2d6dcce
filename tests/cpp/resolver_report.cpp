// The resolver reports through include/iris_hip.hpp: MasksEngine::report and resolver_report.
//   resolver_report <n> <seed> <layout> <threshold> <cap> <k> <nbins>
// The database holds n generated masks (seed); the query is masks_batch.cpp's query 0: limb i ->
// (i + 1) * 0x9E3779B97F4A7C15.  Two participants' share arrays of n * 31 u16:
// share[p][e] = (e * 2654435761 >> 7) + 12345 p (mod 2^16).  MasksEngine::report with all three
// parts runs over records [1, n) with index_base 1000 (the share rows are those of records 1 ..),
// then resolver_report over the same rows against the engine's own rows as denominators, then the
// masks form with the top-k part alone.  Prints what it got, one line per item --
//   form masks | form plain
//   count <matches_count>        m <index> <num> <den> <rotation>     (the matches, ascending)
//   t <index> <num> <den> <rotation>                                  (the k closest, best first)
//   b <nbins words> ...          invalid <count>
//   only <index> ...                                                   (the top-k part alone)
// -- for tests/test_gpu_resolver_report.py to compare with the CPU oracle.  Exit status 0: the calls
// succeeded and the unselected parts of the last call came back empty.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

static bool put(const char *form, const mic::Report &r, uint32_t nbins) {
    if (!r.matches || !r.topk || !r.histogram || r.histogram->bins.size() != nbins) return false;
    std::printf("form %s\ncount %" PRIu64 "\n", form, r.matches->count);
    for (const mic::Match &m : r.matches->list) std::printf("m %" PRIu64 " %u %u %d\n", m.index, m.num, m.den, m.rotation);
    for (const mic::Match &m : *r.topk) std::printf("t %" PRIu64 " %u %u %d\n", m.index, m.num, m.den, m.rotation);
    std::printf("b");
    for (uint64_t b : r.histogram->bins) std::printf(" %" PRIu64, b);
    std::printf("\ninvalid %" PRIu64 "\n", r.histogram->invalid);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s <n> <seed> <layout> <threshold> <cap> <k> <nbins>\n", argv[0]);
        return 2;
    }
    const uint64_t n = (uint64_t)std::atoll(argv[1]), seed = (uint64_t)std::atoll(argv[2]);
    const int layout = std::atoi(argv[3]);
    const double threshold = std::atof(argv[4]);
    const long long cap = std::atoll(argv[5]);
    const uint32_t k = (uint32_t)std::atoi(argv[6]), nbins = (uint32_t)std::atoi(argv[7]);
    if (n < 2) return 2;
    try {
        mic::Device &dev = mic::Device::default_device();
        mic::Database db(dev, IRIS_KIND_MASKS, n, layout);
        db.generate(n, seed, 0);
        mic::Bits query;
        for (std::size_t i = 0; i < query.limbs.size(); ++i) query.limbs[i] = (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
        mic::MasksEngine engine(query, dev);
        const uint64_t rows = n - 1;
        const size_t elems = (size_t)rows * IRIS_ROTATIONS, bytes = elems * sizeof(uint16_t);
        std::vector<uint16_t> share(elems);
        void *dptr[3] = {nullptr, nullptr, nullptr};  // two share arrays, then the engine's rows of records 1 ..
        for (int p = 0; p < 3; ++p) mic::check(iris_device_alloc(dev.handle(), bytes, &dptr[p]));
        for (int p = 0; p < 2; ++p) {
            for (size_t e = 0; e < elems; ++e) share[e] = (uint16_t)(((uint32_t)e * 2654435761u >> 7) + 12345u * (uint32_t)p);
            mic::check(iris_memcpy_h2d(dev.handle(), dptr[p], share.data(), bytes));
        }
        std::vector<mic::Rotations> den(rows);
        engine.batch_process(den, db, 1);
        mic::check(iris_memcpy_h2d(dev.handle(), dptr[2], den[0].data(), bytes));
        const std::vector<const uint16_t *> shares = {(const uint16_t *)dptr[0], (const uint16_t *)dptr[1]};

        mic::ReportRequest req;
        req.threshold = threshold;
        req.cap = cap < 0 ? mic::kAllMatches : (uint64_t)cap;
        req.k = k;
        req.nbins = nbins;
        const mic::Report fused = engine.report(db, shares, req, 1, rows, 1000);
        const mic::Report plain = mic::resolver_report(dev, shares, (const uint16_t *)dptr[2], rows, req, 1000);
        mic::ReportRequest one;
        one.k = k;
        const mic::Report o = engine.report(db, shares, one, 1, rows, 1000);
        for (int p = 0; p < 3; ++p) mic::check(iris_device_free(dev.handle(), dptr[p]));
        if (!put("masks", fused, nbins) || !put("plain", plain, nbins)) return 3;
        if (o.matches || o.histogram || !o.topk) return 3;
        std::printf("only");
        for (const mic::Match &m : *o.topk) std::printf(" %" PRIu64, m.index);
        std::printf("\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
