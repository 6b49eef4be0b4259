// jpegd_rule_main.cpp -- csrc/hs_jpegd_rule.h and nothing else, as a program of its own (tests/test_jpegd_host.py builds
// it with AddressSanitizer and UBSan and runs it as a child process).  Every buffer is allocated exactly to size.
//   jpegd_rule_main all  FILE...   parse and decode every file; all single-byte truncations and 2000 seeded byte flips
//                                  of the first three: decoded or refused, never a report
//   jpegd_rule_main spec S FILE... the speculative procedure of the device decoder on the host: subsequences of S bits
//                                  decoded from guessed states, rounds until nothing changes, must end in the sequential
//                                  decode's exit states, and the write pass from them in the same coefficients
#include <stdio.h>

#include <vector>

#include "hs_jpegd_rule.h"

static std::vector<uint8_t> read_file(const char *path)
{
    std::vector<uint8_t> b;
    FILE *f = fopen(path, "rb");
    if (!f) return b;
    uint8_t tmp[4096];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) b.insert(b.end(), tmp, tmp + n);
    fclose(f);
    return b;
}

// Parse and decode an exact-size copy of data[0 .. n).  Returns decode_host's result, -1 when the header was refused or
// announces a picture this check does not allocate.
static int decode_exact(const uint8_t *data, size_t n, uint32_t *sum)
{
    uint8_t *file = (uint8_t *)malloc(n ? n : 1);
    memcpy(file, data, n);
    hsjpegd::Frame f;
    hsjpegd::Tables *t = (hsjpegd::Tables *)malloc(sizeof(hsjpegd::Tables));
    int r = -1;
    if (hsjpegd::parse(file, n, f, *t, nullptr) == 0 && (long long)f.W * f.H <= (1 << 20)) {
        uint8_t *pix = (uint8_t *)malloc((size_t)f.W * 3u * (size_t)f.H);
        memset(pix, 0, (size_t)f.W * 3u * (size_t)f.H);
        int status = 0;
        r = hsjpegd::decode_host(file, n, 1, pix, (size_t)f.W * 3u, nullptr, &status, nullptr);
        if (r == 0 && sum)
            for (size_t i = 0; i < (size_t)f.W * 3u * (size_t)f.H; i++) *sum = *sum * 31u + pix[i];
        free(pix);
    }
    free(t);
    free(file);
    return r;
}

static int run_all(int nfiles, char **paths)
{
    int decoded = 0, broken_ok = 0, broken_refused = 0;
    uint32_t sum = 0;
    for (int i = 0; i < nfiles; i++) {
        const std::vector<uint8_t> b = read_file(paths[i]);
        if (b.empty() || decode_exact(b.data(), b.size(), &sum) != 0) { printf("FAILED: %s\n", paths[i]); return 1; }
        decoded++;
    }
    uint32_t rng = 12345u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (int i = 0; i < nfiles && i < 3; i++) {
        const std::vector<uint8_t> b = read_file(paths[i]);
        for (size_t n = 0; n < b.size(); n++) (decode_exact(b.data(), n, nullptr) == 0 ? broken_ok : broken_refused)++;
        for (int k = 0; k < 2000; k++) {
            std::vector<uint8_t> c = b;
            c[next() % c.size()] ^= (uint8_t)(1u << (next() % 8u));
            (decode_exact(c.data(), c.size(), nullptr) == 0 ? broken_ok : broken_refused)++;
        }
    }
    printf("jpegd rule ok: %d files, %d broken decoded, %d broken refused, sum %08x\n", decoded, broken_ok, broken_refused, sum);
    return 0;
}

static int run_spec(uint32_t S, int nfiles, char **paths)
{
    int checked = 0, max_rounds = 0;
    for (int i = 0; i < nfiles; i++) {
        const std::vector<uint8_t> b = read_file(paths[i]);
        hsjpegd::Frame f;
        std::vector<hsjpegd::Tables> tv(1);
        const hsjpegd::Tables &t = tv[0];
        if (b.empty() || hsjpegd::parse(b.data(), b.size(), f, tv[0], nullptr)) { printf("FAILED to parse %s\n", paths[i]); return 1; }
        if (f.ri) continue;
        const size_t n = (size_t)f.scan_bytes;
        std::vector<uint32_t> words((n + 8 + 3) / 4);
        size_t nrst = 0;
        const size_t cb = hsjpegd::clean_host(b.data() + f.scan_offset, n, (uint8_t *)words.data(), nullptr, 0, &nrst);
        const uint32_t end = (uint32_t)cb * 8u, nsub = (end + S - 1u) / S;
        // the sequential decode: coefficients, and the state in front of the first symbol at or beyond every boundary
        std::vector<int16_t> want((size_t)f.nblocks * 64u, 0), got((size_t)f.nblocks * 64u, 0);
        std::vector<uint64_t> seq_exit(nsub);
        {
            hsjpegd::State s{0u, 0, 0};
            hsjpegd::NullSink ns;
            for (uint32_t j = 0; j < nsub; j++) {
                while (s.p < (j + 1u) * S) hsjpegd::huff_step(t, f, words.data(), end, s, ns);
                seq_exit[j] = hsjpegd::pack(s);
            }
            hsjpegd::State s0{0u, 0, 0};
            hsjpegd::CoefSink sink{want.data(), 0, f.nblocks};
            if (hsjpegd::decode_stretch(t, f, words.data(), end, s0, end, f.nblocks, sink) || sink.block != f.nblocks) { printf("FAILED: %s does not decode\n", paths[i]); return 1; }
        }
        // the rounds: every lane reads its predecessor's exit of the round before
        std::vector<uint64_t> start(nsub), exit_(nsub), prev;
        std::vector<uint32_t> cnt(nsub);
        for (uint32_t j = 0; j < nsub; j++) {
            hsjpegd::State s{j * S, 0, 0};
            start[j] = hsjpegd::pack(s);
            cnt[j] = hsjpegd::run_subsequence(t, f, words.data(), end, s, (j + 1u) * S);
            exit_[j] = hsjpegd::pack(s);
        }
        int rounds = 0;
        for (bool changed = true; changed; rounds++) {
            changed = false;
            prev = exit_;
            for (uint32_t j = 1; j < nsub; j++)
                if (prev[j - 1] != start[j]) {
                    start[j] = prev[j - 1];
                    hsjpegd::State s = hsjpegd::unpack(start[j]);
                    cnt[j] = hsjpegd::run_subsequence(t, f, words.data(), end, s, (j + 1u) * S);
                    exit_[j] = hsjpegd::pack(s);
                    changed = true;
                }
            if (rounds > (int)nsub) { printf("FAILED: %s S=%u does not settle\n", paths[i], S); return 1; }
        }
        if (exit_ != seq_exit) { printf("FAILED: %s S=%u exit states differ\n", paths[i], S); return 1; }
        int64_t base = 0;
        int status = 0;
        for (uint32_t j = 0; j < nsub; j++) {
            hsjpegd::State s = hsjpegd::unpack(start[j]);
            hsjpegd::CoefSink sink{got.data(), base, f.nblocks};
            const int st = hsjpegd::decode_stretch(t, f, words.data(), end, s, (j + 1u) * S, f.nblocks, sink);
            status = st > status ? st : status;
            base += cnt[j];
        }
        if (status || got != want) { printf("FAILED: %s S=%u coefficients differ (status %d)\n", paths[i], S, status); return 1; }
        max_rounds = rounds > max_rounds ? rounds : max_rounds;
        checked++;
    }
    printf("jpegd spec ok: S=%u, %d files, at most %d rounds\n", S, checked, max_rounds);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "all")) return run_all(argc - 2, argv + 2);
    if (argc >= 4 && !strcmp(argv[1], "spec")) return run_spec((uint32_t)atoi(argv[2]), argc - 3, argv + 3);
    fprintf(stderr, "usage: jpegd_rule_main all FILE... | spec S FILE...\n");
    return 2;
}
