// A masks batch report through include/iris_hip.hpp, as the end of a three-party flow:
//   masks_batch_report <queries> <nq> <n> <seed> <layout> <index_base> <threshold> <cap> <k> <nbins> <out>
// <queries> holds nq raw iris_template_t (3200 B each).  A template database of n generated records
// (seed) is prepared on the device into three parties' share databases and a masks database of
// <layout> (key 0, 1, .., 31); every party's DistanceBatchEngine writes its query-major rows on the
// device, and MasksBatchEngine::report with all three parts runs over them, then the same request
// with the top-k and histogram parts alone, then MasksBatchEngine::resolve.  Writes to <out>, per
// query of the first call: u64 matches count, u64 listed, the listed iris_match_t, u64 top-k count,
// its iris_match_t, the nbins u64 bins, u64 invalid, and resolve()'s iris_match_t -- for
// tests/test_gpu_masks_batch_report.py to compare with the bytes of the C call.  Exit status 0: the
// calls succeeded, the second call's selected parts equal the first's, its matches part came back
// empty, and every query's first top-k entry is resolve()'s record byte for byte.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

int main(int argc, char **argv) {
    if (argc != 12) {
        std::fprintf(stderr, "usage: %s <queries> <nq> <n> <seed> <layout> <index_base> <threshold> <cap> <k> <nbins> <out>\n",
                     argv[0]);
        return 2;
    }
    const size_t nq = (size_t)std::atoll(argv[2]);
    const uint64_t n = std::strtoull(argv[3], nullptr, 10), seed = std::strtoull(argv[4], nullptr, 10);
    const int layout = std::atoi(argv[5]);
    const uint64_t base = std::strtoull(argv[6], nullptr, 10);
    const double threshold = std::atof(argv[7]);
    const uint64_t cap = std::strtoull(argv[8], nullptr, 10);
    const uint32_t k = (uint32_t)std::atoi(argv[9]), nbins = (uint32_t)std::atoi(argv[10]);
    try {
        std::vector<mic::Template> queries(nq);
        std::FILE *in = std::fopen(argv[1], "rb");
        if (!in || std::fread(queries.data(), sizeof(mic::Template), nq, in) != nq) {
            std::fprintf(stderr, "cannot read %zu templates from %s\n", nq, argv[1]);
            return 2;
        }
        std::fclose(in);
        mic::Device &dev = mic::Device::default_device();
        mic::Database templates(dev, IRIS_KIND_TEMPLATES, n, layout), masks(dev, IRIS_KIND_MASKS, n, layout);
        mic::Database s0(dev, IRIS_KIND_SHARES, n), s1(dev, IRIS_KIND_SHARES, n), s2(dev, IRIS_KIND_SHARES, n);
        templates.generate(n, seed, 0);
        std::array<uint8_t, 32> key;
        for (size_t i = 0; i < key.size(); ++i) key[i] = (uint8_t)i;
        mic::prepare_shares(templates, 0, n, key, {&s0, &s1, &s2}, &masks);

        std::vector<mic::EncodedBits> enc;
        std::vector<mic::Bits> qmasks;
        for (const mic::Template &q : queries) {
            enc.push_back(mic::encode(q));
            qmasks.push_back(q.mask);
        }
        const size_t bytes = nq * n * IRIS_ROTATIONS * sizeof(uint16_t);
        void *rows[3] = {nullptr, nullptr, nullptr};
        {
            mic::DistanceBatchEngine de(enc, dev);
            const mic::Database *parties[3] = {&s0, &s1, &s2};
            for (int p = 0; p < 3; ++p) {
                mic::check(iris_device_alloc(dev.handle(), bytes, &rows[p]));
                de.batch_process_device((uint16_t *)rows[p], *parties[p], 0, n);
            }
        }
        const std::vector<const uint16_t *> shares = {(const uint16_t *)rows[0], (const uint16_t *)rows[1],
                                                      (const uint16_t *)rows[2]};
        mic::MasksBatchEngine eng(qmasks, dev);
        mic::ReportRequest req;
        req.threshold = threshold;
        req.cap = cap;
        req.k = k;
        req.nbins = nbins;
        const std::vector<mic::Report> all = eng.report(masks, shares, req, 0, n, base);
        mic::ReportRequest two;
        two.k = k;
        two.nbins = nbins;
        const std::vector<mic::Report> part = eng.report(masks, shares, two, 0, n, base);
        const std::vector<mic::Match> found = eng.resolve(masks, shares, 0, n, base);
        for (int p = 0; p < 3; ++p) mic::check(iris_device_free(dev.handle(), rows[p]));
        if (all.size() != nq || part.size() != nq || found.size() != nq) return 3;

        std::FILE *out = std::fopen(argv[11], "wb");
        if (!out) return 2;
        const auto put = [&](const void *p, size_t len) { return std::fwrite(p, 1, len, out) == len; };
        bool ok = true;
        for (size_t q = 0; q < nq; ++q) {
            const mic::Report &r = all[q], &p = part[q];
            if (!r.matches || !r.topk || !r.histogram || r.histogram->bins.size() != nbins) return 3;
            if (p.matches || !p.topk || !p.histogram) return 3;
            if (p.topk->size() != r.topk->size() || p.histogram->bins != r.histogram->bins ||
                p.histogram->invalid != r.histogram->invalid ||
                std::memcmp(p.topk->data(), r.topk->data(), r.topk->size() * sizeof(mic::Match)) != 0)
                return 4;
            if (r.topk->empty() || std::memcmp(r.topk->data(), &found[q], sizeof(mic::Match)) != 0) return 5;
            const uint64_t listed = r.matches->list.size(), best = r.topk->size();
            ok = ok && put(&r.matches->count, 8) && put(&listed, 8) && put(r.matches->list.data(), listed * sizeof(mic::Match));
            ok = ok && put(&best, 8) && put(r.topk->data(), best * sizeof(mic::Match));
            ok = ok && put(r.histogram->bins.data(), nbins * sizeof(uint64_t)) && put(&r.histogram->invalid, 8);
            ok = ok && put(&found[q], sizeof(mic::Match));
        }
        if (std::fclose(out) != 0 || !ok) return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
