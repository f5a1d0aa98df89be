// Stand-alone check of ogc_amd/csrc/png_unfilter.h for a host sanitizer build (no HIP, no Python):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_unfilter_selftest.cpp -o png_unfilter_selftest
//     ./png_unfilter_selftest
//
// Every filter type at every bpp in exactly-sized heap buffers (a byte read or written outside them is an error of the
// sanitizer), the round trip filter -> unfilter, a one-row image, a filter byte of 5 and the argument refusals.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ogc_amd/csrc/png_unfilter.h"

static int failures = 0;
#define EXPECT(cond)                                                \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);   \
            ++failures;                                             \
        }                                                           \
    } while (0)

static int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the forward filters of the PNG specification on the ORIGINAL neighbours
static std::vector<unsigned char> filter_image(const std::vector<unsigned char> &img, int height, int row_bytes, int bpp,
                                               const std::vector<int> &filters) {
    std::vector<unsigned char> out((size_t)height * (row_bytes + 1));
    for (int y = 0; y < height; ++y) {
        out[(size_t)y * (row_bytes + 1)] = (unsigned char)filters[y];
        for (int x = 0; x < row_bytes; ++x) {
            const int a = x >= bpp ? img[(size_t)y * row_bytes + x - bpp] : 0;
            const int b = y > 0 ? img[(size_t)(y - 1) * row_bytes + x] : 0;
            const int c = (y > 0 && x >= bpp) ? img[(size_t)(y - 1) * row_bytes + x - bpp] : 0;
            const int pred[5] = {0, a, b, (a + b) >> 1, paeth(a, b, c)};
            out[(size_t)y * (row_bytes + 1) + 1 + x] = (unsigned char)(img[(size_t)y * row_bytes + x] - pred[filters[y]]);
        }
    }
    return out;
}

int main() {
    unsigned seed = 12345u;
    auto next = [&seed]() { seed = seed * 1664525u + 1013904223u; return (unsigned char)(seed >> 24); };
    const int bpps[4] = {1, 2, 3, 6};
    for (int bpp : bpps) {
        for (int height : {1, 2, 7}) {
            for (int width : {1, 2, 13}) {
                const int row_bytes = width * bpp;
                std::vector<unsigned char> img((size_t)height * row_bytes);
                for (auto &v : img) v = next();
                img[0] = 255;
                for (int variant = 0; variant < 6; ++variant) { // one filter type for all rows, then mixed
                    std::vector<int> filters(height);
                    for (int y = 0; y < height; ++y) filters[y] = variant < 5 ? variant : (y * 3 + 4) % 5;
                    const std::vector<unsigned char> in = filter_image(img, height, row_bytes, bpp, filters);
                    std::vector<unsigned char> out((size_t)height * row_bytes, 0xAB);
                    int bad = -1;
                    EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), height, row_bytes, bpp, &bad) == OGC_PNG_OK);
                    EXPECT(out == img);
                }
            }
        }
    }
    {   // a filter byte of 5 in the third row: the rows in front are written, the status names the row
        const int height = 4, row_bytes = 12, bpp = 6;
        std::vector<unsigned char> in((size_t)height * (row_bytes + 1), 1), out((size_t)height * row_bytes, 0xAB);
        in[2 * (row_bytes + 1)] = 5;
        int bad = -1;
        EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), height, row_bytes, bpp, &bad) == OGC_PNG_FILTER);
        EXPECT(bad == 2);
        EXPECT(out[2 * row_bytes] == 0xAB && out[2 * row_bytes - 1] != 0xAB);
        in[2 * (row_bytes + 1)] = 255;
        EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), height, row_bytes, bpp, &bad) == OGC_PNG_FILTER);
    }
    {   // refusals: nothing is read or written
        std::vector<unsigned char> in(15, 0), out(14, 0xAB);
        EXPECT(ogc_png_unfilter_rows(nullptr, out.data(), 1, 14, 2, nullptr) == OGC_PNG_NULL);
        EXPECT(ogc_png_unfilter_rows(in.data(), nullptr, 1, 14, 2, nullptr) == OGC_PNG_NULL);
        EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), -1, 14, 2, nullptr) == OGC_PNG_SIZE);
        EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), 1, -14, 2, nullptr) == OGC_PNG_SIZE);
        for (int bpp : {0, 4, 5, 7, 8, -1}) EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), 1, 14, bpp, nullptr) == OGC_PNG_BPP);
        EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), 1, 14, 3, nullptr) == OGC_PNG_ROW_BYTES);
        EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), 1, 14, 6, nullptr) == OGC_PNG_ROW_BYTES);
        EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), 0, 14, 2, nullptr) == OGC_PNG_OK);
        for (unsigned char v : out) EXPECT(v == 0xAB);
        in[0] = 9; // a bad filter byte with no place to report the row
        EXPECT(ogc_png_unfilter_rows(in.data(), out.data(), 1, 14, 2, nullptr) == OGC_PNG_FILTER);
    }
    std::printf(failures ? "png_unfilter_selftest: %d FAILURES\n" : "png_unfilter_selftest: all checks passed\n", failures);
    return failures ? 1 : 0;
}
