// CompressorImpl's footer (flate_hip_checksum per piece, flate_hip_checksum_combine between them) on all-0xFF data written in
// pieces with a flush after each.  Needs a GPU to run.  Prints, per stream, the container, the number of plain bytes and the
// footer bytes in hex; tests/test_gpu_checksums.py compares them with zlib's.
#include <cstdio>
#include <cstdlib>

#include "../../flate_amd/host/flate.hpp"

using namespace flate_hip;

static const size_t PIECES[] = {1, 65520, 65521, 65535, 65536};

template <class C>
static size_t feed(C& c, const std::vector<uint8_t>& ff, int rounds) {
    size_t total = 0;
    for (int r = 0; r < rounds; r++)
        for (size_t n : PIECES) {
            c.write(ff.data(), n);
            c.flush();
            total += n;
        }
    c.finish();
    return total;
}

static void report(const char* name, size_t total, const std::vector<uint8_t>& out, size_t nfoot) {
    printf("%s %zu ", name, total);
    for (size_t i = out.size() - nfoot; i < out.size(); i++) printf("%02x", out[i]);
    printf("\n");
}

int main() {
    const std::vector<uint8_t> ff(65536, 0xff);
    for (int rounds : {1, 3}) {
        {
            VectorWriter w;
            auto c = gzip::compressor(w);
            report("gzip", feed(c, ff, rounds), w.data, 8);
        }
        {
            VectorWriter w;
            auto c = zlib::compressor(w);
            report("zlib", feed(c, ff, rounds), w.data, 4);
        }
        {
            VectorWriter w;
            auto c = gzip::huffman::compressor(w);
            report("gzip", feed(c, ff, rounds), w.data, 8);
        }
        {
            VectorWriter w;
            auto c = zlib::store::compressor(w);
            report("zlib", feed(c, ff, rounds), w.data, 4);
        }
    }
    printf("checksum flush ok\n");
    return 0;
}
