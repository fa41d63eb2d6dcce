// A combined pass through include/iris_hip.hpp on a generated database:
//   report <n> <seed> <layout> <threshold> <cap> <k> <nbins>
// A database of n generated templates (seed); the query is generated template 0 of seed + 1.
// TemplateEngine::report with all three parts runs over records [1, n) with index_base 1000, and the
// same request with the top-k part alone.  Prints what it got, one line per item --
//   count <matches_count>        m <index> <num> <den> <rotation>     (the matches, ascending)
//   t <index> <num> <den> <rotation>                                  (the k closest, best first)
//   b <nbins words> ...          invalid <count>
//   only <index> ...                                                   (the top-k part alone)
// -- for tests/test_gpu_report.py to compare with the CPU oracle.  Exit status 0: the calls succeeded
// and the unselected parts of the second call came back empty.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

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
    try {
        mic::Device &dev = mic::Device::default_device();
        mic::Database tdb(dev, IRIS_KIND_TEMPLATES, n, layout);
        tdb.generate(n, seed, 0);
        mic::Database qdb(dev, IRIS_KIND_TEMPLATES, 1, layout);
        qdb.generate(1, seed + 1, 0);
        iris_template_t raw;
        mic::check(iris_db_read(qdb.handle(), 0, 1, &raw));
        mic::Template query;
        std::memcpy(query.pattern.limbs.data(), raw.pattern, sizeof raw.pattern);
        std::memcpy(query.mask.limbs.data(), raw.mask, sizeof raw.mask);
        mic::TemplateEngine te(query, dev);

        mic::ReportRequest req;
        req.threshold = threshold;
        req.cap = cap < 0 ? mic::kAllMatches : (uint64_t)cap;
        req.k = k;
        req.nbins = nbins;
        const mic::Report r = te.report(tdb, req, 1, n - 1, 1000);
        if (!r.matches || !r.topk || !r.histogram || r.histogram->bins.size() != nbins) return 3;
        std::printf("count %" PRIu64 "\n", r.matches->count);
        for (const mic::Match &m : r.matches->list)
            std::printf("m %" PRIu64 " %u %u %d\n", m.index, m.num, m.den, m.rotation);
        for (const mic::Match &m : *r.topk) std::printf("t %" PRIu64 " %u %u %d\n", m.index, m.num, m.den, m.rotation);
        std::printf("b");
        for (uint64_t b : r.histogram->bins) std::printf(" %" PRIu64, b);
        std::printf("\ninvalid %" PRIu64 "\n", r.histogram->invalid);

        mic::ReportRequest one;
        one.k = k;
        const mic::Report o = te.report(tdb, one, 1, n - 1, 1000);
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
