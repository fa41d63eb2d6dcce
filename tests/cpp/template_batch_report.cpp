// A template batch report through include/iris_hip.hpp on records the caller gives:
//   template_batch_report <templates> <n> <queries> <nq> <layout> <first> <count> <index_base>
//                         <threshold> <cap> <k> <nbins> <out>
// <templates> and <queries> hold n and nq raw iris_template_t (3200 B each).  A database of capacity
// n + 43 takes the templates; TemplateBatchEngine::report with all three parts runs over records
// [first, first + count), and the same request with the top-k and histogram parts alone.  Writes to
// <out>, per query of the first call: u64 matches count, u64 listed, the listed iris_match_t, u64
// top-k count, its iris_match_t, the nbins u64 bins, u64 invalid -- for
// tests/test_gpu_template_batch_report.py to compare with the bytes of the C call.  Exit status 0:
// the calls succeeded, the second call's selected parts equal the first's and its matches part
// came back empty.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

static std::vector<mic::Template> read_templates(const char *path, size_t n) {
    std::vector<mic::Template> v(n);
    std::FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(mic::Template), n, f) != n) {
        std::fprintf(stderr, "cannot read %zu templates from %s\n", n, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 14) {
        std::fprintf(stderr, "usage: %s <templates> <n> <queries> <nq> <layout> <first> <count> <index_base> <threshold> "
                             "<cap> <k> <nbins> <out>\n", argv[0]);
        return 2;
    }
    const size_t n = (size_t)std::atoll(argv[2]), nq = (size_t)std::atoll(argv[4]);
    const int layout = std::atoi(argv[5]);
    const uint64_t first = std::strtoull(argv[6], nullptr, 10), count = std::strtoull(argv[7], nullptr, 10);
    const uint64_t base = std::strtoull(argv[8], nullptr, 10);
    const double threshold = std::atof(argv[9]);
    const uint64_t cap = std::strtoull(argv[10], nullptr, 10);
    const uint32_t k = (uint32_t)std::atoi(argv[11]), nbins = (uint32_t)std::atoi(argv[12]);
    try {
        const std::vector<mic::Template> templates = read_templates(argv[1], n), queries = read_templates(argv[3], nq);
        mic::Device &dev = mic::Device::default_device();
        mic::Database db(dev, IRIS_KIND_TEMPLATES, n + 43, layout);
        db.append(templates);
        mic::TemplateBatchEngine eng(queries, dev);

        mic::ReportRequest req;
        req.threshold = threshold;
        req.cap = cap;
        req.k = k;
        req.nbins = nbins;
        const std::vector<mic::Report> all = eng.report(db, req, first, count, base);
        mic::ReportRequest two;
        two.k = k;
        two.nbins = nbins;
        const std::vector<mic::Report> part = eng.report(db, two, first, count, base);
        if (all.size() != nq || part.size() != nq) return 3;

        std::FILE *out = std::fopen(argv[13], "wb");
        if (!out) return 2;
        const auto put = [&](const void *p, size_t bytes) { return std::fwrite(p, 1, bytes, out) == bytes; };
        bool ok = true;
        for (size_t q = 0; q < nq; ++q) {
            const mic::Report &r = all[q], &p = part[q];
            if (!r.matches || !r.topk || !r.histogram || r.histogram->bins.size() != nbins) return 3;
            if (p.matches || !p.topk || !p.histogram) return 3;
            if (p.topk->size() != r.topk->size() || p.histogram->bins != r.histogram->bins ||
                p.histogram->invalid != r.histogram->invalid ||
                std::memcmp(p.topk->data(), r.topk->data(), r.topk->size() * sizeof(mic::Match)) != 0)
                return 4;
            const uint64_t listed = r.matches->list.size(), best = r.topk->size();
            ok = ok && put(&r.matches->count, 8) && put(&listed, 8) && put(r.matches->list.data(), listed * sizeof(mic::Match));
            ok = ok && put(&best, 8) && put(r.topk->data(), best * sizeof(mic::Match));
            ok = ok && put(r.histogram->bins.data(), nbins * sizeof(uint64_t)) && put(&r.histogram->invalid, 8);
        }
        if (std::fclose(out) != 0 || !ok) return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
