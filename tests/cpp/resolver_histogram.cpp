// The resolver histograms through include/iris_hip.hpp: MasksBatchEngine::histogram,
// MasksEngine::histogram and resolver_histogram.
//   resolver_histogram <out file> <nq> <n> <seed> <layout> <nbins>
// The database holds n generated masks (seed); query q is masks_batch.cpp's: limb i ->
// (i + 1) * 0x9E3779B97F4A7C15 * (2 q + 1) ^ (q << 7).  Two participants' query-major share arrays
// of nq * n * 31 u16: share[p][e] = (e * 2654435761 >> 7) + 12345 p (mod 2^16).  The out file
// receives, as u64: per query the nbins bins and the invalid count of the batched call; then per
// query those of MasksEngine(query q) on slab q; then per query those of resolver_histogram on slab
// q against the batch engine's own rows as denominators.
// tests/test_gpu_resolver_histogram.py compares them with the CPU oracle.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

static bool put(std::FILE *f, const mic::Histogram &h) {
    return std::fwrite(h.bins.data(), sizeof(uint64_t), h.bins.size(), f) == h.bins.size() &&
           std::fwrite(&h.invalid, sizeof h.invalid, 1, f) == 1;
}

int main(int argc, char **argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s <out file> <nq> <n> <seed> <layout> <nbins>\n", argv[0]);
        return 2;
    }
    const uint32_t nq = (uint32_t)std::atoi(argv[2]);
    const uint64_t n = (uint64_t)std::atoll(argv[3]), seed = (uint64_t)std::atoll(argv[4]);
    const int layout = std::atoi(argv[5]);
    const uint32_t nbins = (uint32_t)std::atoi(argv[6]);
    try {
        mic::Device &dev = mic::Device::default_device();
        mic::Database db(dev, IRIS_KIND_MASKS, n, layout);
        db.generate(n, seed, 0);
        std::vector<mic::Bits> queries(nq);
        for (uint32_t q = 0; q < nq; ++q)
            for (std::size_t i = 0; i < queries[q].limbs.size(); ++i)
                queries[q].limbs[i] = ((uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull * (2 * q + 1)) ^ ((uint64_t)q << 7);
        mic::MasksBatchEngine engine(queries, dev);
        const size_t slab = (size_t)n * IRIS_ROTATIONS, elems = (size_t)nq * slab, bytes = elems * sizeof(uint16_t);
        std::vector<uint16_t> share(elems);
        void *dptr[3] = {nullptr, nullptr, nullptr};  // two share arrays, then the engine's rows
        for (int p = 0; p < 3; ++p) mic::check(iris_device_alloc(dev.handle(), bytes, &dptr[p]));
        for (int p = 0; p < 2; ++p) {
            for (size_t e = 0; e < elems; ++e) share[e] = (uint16_t)(((uint32_t)e * 2654435761u >> 7) + 12345u * (uint32_t)p);
            mic::check(iris_memcpy_h2d(dev.handle(), dptr[p], share.data(), bytes));
        }
        engine.batch_process_device((uint16_t *)dptr[2], db, 0, n);
        const std::vector<const uint16_t *> shares = {(const uint16_t *)dptr[0], (const uint16_t *)dptr[1]};
        const std::vector<mic::Histogram> batch = engine.histogram(db, shares, nbins, 0, n);
        std::vector<mic::Histogram> single, plain;
        for (uint32_t q = 0; q < nq; ++q) {
            const std::vector<const uint16_t *> sl = {shares[0] + q * slab, shares[1] + q * slab};
            single.push_back(mic::MasksEngine(queries[q], dev).histogram(db, sl, nbins, 0, n));
            plain.push_back(mic::resolver_histogram(dev, sl, (const uint16_t *)dptr[2] + q * slab, n, nbins));
        }
        for (int p = 0; p < 3; ++p) mic::check(iris_device_free(dev.handle(), dptr[p]));
        if (batch.size() != nq) return 3;
        for (uint32_t q = 0; q < nq; ++q)
            if (batch[q].bins.size() != nbins || single[q].bins.size() != nbins || plain[q].bins.size() != nbins) return 3;

        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 4;
        bool ok = true;
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, batch[q]);
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, single[q]);
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, plain[q]);
        std::fclose(f);
        return ok ? 0 : 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
