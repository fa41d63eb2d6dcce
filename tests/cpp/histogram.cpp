// Distance histograms through include/iris_hip.hpp on a generated database:
//   histogram <expected file> <n> <seed> <layout> <nbins> <nq>
// A database of n generated templates (seed); the queries are generated templates 0 .. nq - 1 of
// seed + 1.  TemplateEngine::histogram of query 0 runs over records [1, n), and
// TemplateBatchEngine::histogram of all nq queries over the same range.
// The expected file holds, as u64: the single histogram's nbins bins and its invalid count, then
// the batch call's nq * nbins bins (query-major) and its nq invalid counts -- written by
// tests/test_gpu_template_batch_histogram.py from the CPU oracle.  Exit status 0: every word equal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

int main(int argc, char **argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s <expected file> <n> <seed> <layout> <nbins> <nq>\n", argv[0]);
        return 2;
    }
    const uint64_t n = (uint64_t)std::atoll(argv[2]), seed = (uint64_t)std::atoll(argv[3]);
    const int layout = std::atoi(argv[4]);
    const uint32_t nbins = (uint32_t)std::atoi(argv[5]), nq = (uint32_t)std::atoi(argv[6]);
    try {
        std::vector<uint64_t> want((size_t)(nbins + 1) * (1 + nq));
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 4;
        const size_t got_words = std::fread(want.data(), sizeof(uint64_t), want.size(), f);
        std::fclose(f);
        if (got_words != want.size()) return 4;

        mic::Device &dev = mic::Device::default_device();
        mic::Database tdb(dev, IRIS_KIND_TEMPLATES, n, layout);
        tdb.generate(n, seed, 0);
        mic::Database qdb(dev, IRIS_KIND_TEMPLATES, nq, layout);
        qdb.generate(nq, seed + 1, 0);
        std::vector<iris_template_t> raw(nq);
        mic::check(iris_db_read(qdb.handle(), 0, nq, raw.data()));
        std::vector<mic::Template> queries(nq);
        for (uint32_t q = 0; q < nq; ++q) {
            std::memcpy(queries[q].pattern.limbs.data(), raw[q].pattern, sizeof raw[q].pattern);
            std::memcpy(queries[q].mask.limbs.data(), raw[q].mask, sizeof raw[q].mask);
        }

        std::vector<uint64_t> got;
        mic::TemplateEngine te(queries[0], dev);
        const mic::Histogram one = te.histogram(tdb, nbins, 1, n - 1);
        if (one.bins.size() != nbins) return 3;
        got.insert(got.end(), one.bins.begin(), one.bins.end());
        got.push_back(one.invalid);
        mic::TemplateBatchEngine be(queries, dev);
        const std::vector<mic::Histogram> all = be.histogram(tdb, nbins, 1, n - 1);
        if (all.size() != nq) return 3;
        for (const mic::Histogram &h : all) {
            if (h.bins.size() != nbins) return 3;
            got.insert(got.end(), h.bins.begin(), h.bins.end());
        }
        for (const mic::Histogram &h : all) got.push_back(h.invalid);
        for (size_t i = 0; i < want.size(); ++i)
            if (got[i] != want[i]) {
                std::fprintf(stderr, "word %zu: got %llu, expected %llu\n", i, (unsigned long long)got[i],
                             (unsigned long long)want[i]);
                return 5;
            }
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
