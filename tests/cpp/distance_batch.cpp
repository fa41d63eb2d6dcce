// A DistanceBatchEngine (include/iris_hip.hpp) on a generated share database:
//   distance_batch <out file> <nq> <n> <seed> <layout>
// Query q is element i -> (uint16)(i * (2 q + 3) + 7 q + (i >> 3)); the database holds n + 57
// generated shares and the batch runs over records [57, 57 + n).  The nq * n rows of 31 u16
// (query-major) are written to <out file>; tests/test_gpu_distance_batch.py compares them with
// the rows the Python side computes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

int main(int argc, char **argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <out file> <nq> <n> <seed> <layout>\n", argv[0]);
        return 2;
    }
    const uint32_t nq = (uint32_t)std::atoi(argv[2]);
    const uint64_t n = (uint64_t)std::atoll(argv[3]), seed = (uint64_t)std::atoll(argv[4]);
    const int layout = std::atoi(argv[5]);
    try {
        mic::Device &dev = mic::Device::default_device();
        mic::Database db(dev, IRIS_KIND_SHARES, n + 57, layout);
        db.generate(n + 57, seed, 0);
        std::vector<mic::EncodedBits> queries(nq);
        for (uint32_t q = 0; q < nq; ++q)
            for (std::size_t i = 0; i < mic::BITS; ++i) queries[q].v[i] = (uint16_t)(i * (2 * q + 3) + 7 * q + (i >> 3));
        mic::DistanceBatchEngine engine(queries, dev);
        if (engine.nq() != nq) return 3;
        std::vector<mic::Rotations> out;
        engine.batch_process(out, db, 57, n);
        if (out.size() != (std::size_t)nq * n) return 3;
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 4;
        const std::size_t wrote = std::fwrite(out.data(), sizeof(mic::Rotations), out.size(), f);
        std::fclose(f);
        return wrote == out.size() ? 0 : 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
