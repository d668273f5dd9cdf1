// tests/tools/spz_sanitize.cpp — a stand-alone program over csrc/spz_container.hpp (which includes nothing of HIP) for a sanitizer
// run by hand: every file named on the command line is inflated and its container parsed; of a file that opens, every plane
// byte of every splat is read through the layout the device staging and the host image builder use.  Prints one line per
// file; the exit status is 0 whatever was refused - a sanitizer report is what fails the run.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gaussiansplats3d_amd/csrc \
//       tests/tools/spz_sanitize.cpp -o spz_sanitize && ./spz_sanitize good.spz damaged-*.spz
#include <stdio.h>

#include "spz_container.hpp"

int main(int argc, char** argv) {
    int opened = 0, refused = 0;
    for (int k = 1; k < argc; k++) {
        FILE* f = fopen(argv[k], "rb");
        if (!f) { printf("%s: cannot be read\n", argv[k]); continue; }
        std::vector<uint8_t> data;
        uint8_t chunk[65536];
        for (size_t got; (got = fread(chunk, 1, sizeof(chunk), f)) > 0;) data.insert(data.end(), chunk, chunk + got);
        fclose(f);
        // an exact-size heap copy: a read one byte past the input is a report
        std::vector<uint8_t> exact(data.begin(), data.end());
        exact.shrink_to_fit();
        std::vector<uint8_t> stream;
        SpzHeader h;
        const char* why = spz_open(exact.data(), exact.size(), stream, h);
        if (why) { refused++; printf("%s: refused: %s\n", argv[k], why); continue; }
        opened++;
        std::vector<uint8_t> planes(stream.begin(), stream.end());      // exact size again
        planes.shrink_to_fit();
        uint64_t sum = 0;
        for (uint32_t i = 0; i < h.count; i++)
            for (int p = 0; p < SPZ_PLANES; p++) {
                const uint32_t stride = spz_plane_stride(h.layout, p);
                const uint8_t* at = planes.data() + h.layout.off[p] + (size_t)stride * i;
                for (uint32_t b = 0; b < stride; b++) sum += at[b];
            }
        printf("%s: version %u, %u splats, SH degree %u, fractionalBits %u, position scale %g, %llu bytes, byte sum %llu\n", argv[k], h.version,
               h.count, h.sh_degree, h.fractional_bits, h.layout.pos_scale, (unsigned long long)h.stream_bytes, (unsigned long long)sum);
    }
    printf("%d opened, %d refused\n", opened, refused);
    return 0;
}
