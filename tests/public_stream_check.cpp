// Stand-alone host check of public stream v1 (csrc/wire/wire.hpp): prints the
// words host::public_stream_v1 draws, for tests/test_wire_seeded.py to compare
// with the numpy restatement (tests/wire_seeded_spec.py).  Built with
// -fsanitize=address,undefined by the test; host only.
//
//   public_stream_check SEEDHEX KID DIGIT FIRST N Q...
//
// prints one line per prime, limb index FIRST + i: N words in hex.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fhe-sorting_amd/csrc/host/hostmath.hpp"

int main(int argc, char **argv) {
    if (argc < 7 || std::strlen(argv[1]) != 64) {
        std::fprintf(stderr, "usage: %s SEEDHEX(64) KID DIGIT FIRST N Q...\n", argv[0]);
        return 2;
    }
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) {
        unsigned b = 0;
        if (std::sscanf(argv[1] + 2 * i, "%2x", &b) != 1) return 2;
        seed[i] = (uint8_t)b;
    }
    const fhe::host::u64 kid = std::strtoull(argv[2], nullptr, 10);
    const int digit = std::atoi(argv[3]);
    const size_t first = std::strtoull(argv[4], nullptr, 10), n = std::strtoull(argv[5], nullptr, 10);
    // the stream indexes primes by their position in the chain: pad below `first`
    std::vector<fhe::host::u64> primes(first, 0);
    for (int i = 6; i < argc; ++i) primes.push_back(std::strtoull(argv[i], nullptr, 10));
    const size_t limbs = primes.size() - first;
    std::vector<fhe::host::u64> out(limbs * n);
    if (!fhe::host::public_stream_v1(seed, kid, digit, primes.data(), first, limbs, n, out.data())) {
        std::printf("exhausted\n");
        return 1;
    }
    for (size_t l = 0; l < limbs; ++l) {
        for (size_t k = 0; k < n; ++k) std::printf("%llx%c", (unsigned long long)out[l * n + k], k + 1 == n ? '\n' : ' ');
    }
    return 0;
}
