// _gif_san_main.cpp -- TEST INFRASTRUCTURE: the host build of the GIF decoder (oracle/keyes_gif_cpu.cpp) as a program of its own,
// so that tests/test_gif_cpu.py can run it under AddressSanitizer and UBSan with the sanitiser's runtime linked in.  Reads a
// list of file paths; per file decodes directly, then through the kernels' sink and the replay of its records -- the file
// without a byte of slack, the indices with the one byte the sink may write behind them, the records as many as the kernel
// reserves -- and prints "<status> <Adler-32 of the pixels> <status> <Adler-32>" for the two ways.
#include <cstdio>
#include <string>

#include "../oracle/keyes_gif_cpu.cpp"

static uint32_t adler32(const uint8_t *p, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t k = 0; k < n; ++k) {
        a = (a + p[k]) % 65521u;
        b = (b + a) % 65521u;
    }
    return (b << 16) | a;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *list = std::fopen(argv[1], "r");
    if (!list) return 2;
    char path[4096];
    while (std::fscanf(list, "%4095s", path) == 1) {
        FILE *f = std::fopen(path, "rb");
        if (!f) return 2;
        std::vector<uint8_t> data;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
        std::fclose(f);
        std::vector<uint8_t> exact(data.begin(), data.end());          // no slack behind the file's last byte
        int32_t w = 0, h = 0, ch = 0;
        int st = ko_gif_probe(exact.data(), exact.size(), &w, &h, &ch), st2 = st;
        uint32_t sum = 1, sum2 = 1;
        if (st == 0) {
            const size_t want = (size_t)w * h;
            std::vector<uint8_t> out(want), out2(want), idx(want + 1);
            st = ko_gif_decode(exact.data(), exact.size(), out.data());
            if (st == 0) sum = adler32(out.data(), want);
            std::vector<uint32_t> rec(2 * (want / 2 + 2));             // the bound of ke_gif.hip: a record more is a report
            uint32_t nrec = 0;
            st2 = ko_gif_records(exact.data(), exact.size(), idx.data(), rec.data(), &nrec);
            if (st2 == 0) st2 = ko_gif_replay(exact.data(), exact.size(), idx.data(), rec.data(), nrec, out2.data());
            if (st2 == 0) sum2 = adler32(out2.data(), want);
        }
        std::printf("%d %u %d %u\n", st, sum, st2, sum2);
    }
    std::fclose(list);
    return 0;
}
