// png_unfilter.h — the row filters of a PNG undone (PNG specification, section 9: None, Sub, Up, Average, Paeth).  Plain C++, no
// HIP: Average and Paeth need the reconstructed byte to the left and the reconstructed row above, so the work is sequential per
// byte — nothing for numpy, nothing for a GPU.  ogc_amd/data_prepare/png16.py calls it through ogc_png_unfilter (api.hip).
#pragma once

enum {
    OGC_PNG_OK = 0,
    OGC_PNG_NULL = 1,      // in or out is null
    OGC_PNG_SIZE = 2,      // height or row_bytes negative
    OGC_PNG_BPP = 3,       // bytes per pixel not in {1, 2, 3, 6}: grey or RGB at 8 or 16 bits
    OGC_PNG_ROW_BYTES = 4, // row_bytes is no multiple of bpp
    OGC_PNG_FILTER = 5     // a filter byte above 4; *bad_row is the row
};

// in: height rows of (1 filter byte + row_bytes filtered bytes); out: height * row_bytes reconstructed bytes.  bpp is the PNG's
// "bytes per complete pixel".  Bytes left of the row and the row above the first count as zero.  Rows before a bad filter byte
// are written, the others are not.
static inline int ogc_png_unfilter_rows(const unsigned char *in, unsigned char *out, int height, int row_bytes, int bpp,
                                        int *bad_row) {
    if (!in || !out) return OGC_PNG_NULL;
    if (height < 0 || row_bytes < 0) return OGC_PNG_SIZE;
    if (bpp != 1 && bpp != 2 && bpp != 3 && bpp != 6) return OGC_PNG_BPP;
    if (row_bytes % bpp != 0) return OGC_PNG_ROW_BYTES;
    for (int y = 0; y < height; ++y) {
        const unsigned char *src = in + (long long)y * (row_bytes + 1);
        unsigned char *cur = out + (long long)y * row_bytes;
        const unsigned char *up = y > 0 ? cur - row_bytes : nullptr;
        const int filter = src[0];
        ++src;
        switch (filter) {
        case 0:
            for (int x = 0; x < row_bytes; ++x) cur[x] = src[x];
            break;
        case 1:
            for (int x = 0; x < row_bytes; ++x) cur[x] = (unsigned char)(src[x] + (x >= bpp ? cur[x - bpp] : 0));
            break;
        case 2:
            for (int x = 0; x < row_bytes; ++x) cur[x] = (unsigned char)(src[x] + (up ? up[x] : 0));
            break;
        case 3:
            for (int x = 0; x < row_bytes; ++x) {
                const int a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0;
                cur[x] = (unsigned char)(src[x] + ((a + b) >> 1));
            }
            break;
        case 4:
            for (int x = 0; x < row_bytes; ++x) {
                const int a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
                const int p = a + b - c;
                const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
                const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                cur[x] = (unsigned char)(src[x] + pred);
            }
            break;
        default:
            if (bad_row) *bad_row = y;
            return OGC_PNG_FILTER;
        }
    }
    return OGC_PNG_OK;
}
