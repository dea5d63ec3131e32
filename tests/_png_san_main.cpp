// _png_san_main.cpp -- TEST INFRASTRUCTURE: the host build of the PNG decoder (oracle/keyes_png_cpu.cpp) as a program of its own,
// so that tests/test_png_cpu.py can run it under AddressSanitizer and UBSan with the sanitiser's runtime linked in.
// Reads a list of file paths; prints per file "<status> <Adler-32 of the pixels>".
#include <cstdio>
#include <string>

#include "../oracle/keyes_png_cpu.cpp"

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
        const size_t size = data.size();
        data.push_back(0);
        int32_t w = 0, h = 0, ch = 0;
        int st = ko_png_probe(data.data(), size, &w, &h, &ch);
        uint32_t sum = 1;
        if (st == 0) {
            std::vector<uint8_t> out((size_t)w * h * ch);             // exactly the pixels: a byte more written is a report
            st = ko_png_decode(data.data(), size, out.data());
            if (st == 0) sum = ke_adler32(out.data(), out.size());
        }
        std::printf("%d %u\n", st, sum);
    }
    std::fclose(list);
    return 0;
}
