// make_golden_triangulate_eigen.cc -- our own generator of tests/golden/tri_eigen.npz: what a compiled Eigen::JacobiSVD<Matrix4f> gives on the
// 4 x 4 matrices of tests/triangulate_cases.py, so that tests/test_tri_eigen_golden.py can hold the fixed text of csrc/tri_math.h against it
// (until then the parity is unpinned).  For a machine that has Eigen 3; nothing here is built by this repository.
//
//   python -c "from tests import triangulate_cases as TC; TC.write_svd_inputs('tri_svd_in.bin')"
//   g++ -O2 -std=c++14 -ffp-contract=off -I /usr/include/eigen3 tools/make_golden_triangulate_eigen.cc -o make_golden_triangulate_eigen
//   ./make_golden_triangulate_eigen tri_svd_in.bin tests/golden/tri_eigen.npz
//
// Input: int32 n | float A[n][16] row-major.  Output, an uncompressed .npz: A (n, 4, 4), V (n, 4, 4) = SVD.matrixV(), x3D (n, 3) =
// V.block<3, 1>(0, 3) / V(3, 3) as src/LocalMapping.cc:1106-1110 writes it (inf / NaN where V(3, 3) == 0), version (3,) = EIGEN_WORLD / MAJOR /
// MINOR_VERSION.  Build it the way the SLAM system is built if its flags are known (-march=native lets Eigen vectorise the rotations).
#include <Eigen/Dense>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

uint32_t crc32(const std::string &s) {
    static uint32_t table[256];
    if (!table[1])
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    uint32_t c = 0xFFFFFFFFu;
    for (unsigned char b : s) c = table[(c ^ b) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
void put16(std::string &o, uint16_t v) { o.append((const char *) &v, 2); }
void put32(std::string &o, uint32_t v) { o.append((const char *) &v, 4); }

// one array as a .npy (format 1.0, little endian)
std::string npy(const char *descr, const std::vector<size_t> &shape, const void *data, size_t bytes) {
    std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (";
    for (size_t d : shape) dict += std::to_string(d) + ",";
    dict += "), }";
    while ((10 + dict.size() + 1) % 64) dict += ' ';
    dict += '\n';
    std::string o("\x93NUMPY\x01\x00", 8);
    put16(o, (uint16_t) dict.size());
    o += dict;
    o.append((const char *) data, bytes);
    return o;
}

struct Entry { std::string name, body; uint32_t crc, offset; };

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: make_golden_triangulate_eigen in.bin out.npz\n"); return 2; }
    FILE *in = std::fopen(argv[1], "rb");
    int32_t n = 0;
    if (!in || std::fread(&n, 4, 1, in) != 1 || n <= 0) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<float> A((size_t) n * 16), V((size_t) n * 16), X((size_t) n * 3);
    if (std::fread(A.data(), 4, A.size(), in) != A.size()) { std::fprintf(stderr, "short read\n"); return 2; }
    std::fclose(in);
    for (int k = 0; k < n; k++) {
        Eigen::Matrix4f M;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) M(r, c) = A[(size_t) k * 16 + 4 * r + c];
        Eigen::JacobiSVD<Eigen::Matrix4f> SVD(M, Eigen::ComputeFullU | Eigen::ComputeFullV);
        const Eigen::Matrix4f v = SVD.matrixV();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) V[(size_t) k * 16 + 4 * r + c] = v(r, c);
        const Eigen::Vector3f x = v.block<3, 1>(0, 3) / v(3, 3);
        for (int a = 0; a < 3; a++) X[(size_t) k * 3 + a] = x[a];
    }
    const int32_t version[3] = {EIGEN_WORLD_VERSION, EIGEN_MAJOR_VERSION, EIGEN_MINOR_VERSION};
    std::vector<Entry> entries;
    entries.push_back({"A.npy", npy("<f4", {(size_t) n, 4, 4}, A.data(), A.size() * 4), 0, 0});
    entries.push_back({"V.npy", npy("<f4", {(size_t) n, 4, 4}, V.data(), V.size() * 4), 0, 0});
    entries.push_back({"x3D.npy", npy("<f4", {(size_t) n, 3}, X.data(), X.size() * 4), 0, 0});
    entries.push_back({"version.npy", npy("<i4", {3}, version, sizeof version), 0, 0});
    std::string zip, central;
    for (Entry &e : entries) {
        e.crc = crc32(e.body);
        e.offset = (uint32_t) zip.size();
        put32(zip, 0x04034b50u); put16(zip, 20); put16(zip, 0); put16(zip, 0); put16(zip, 0); put16(zip, 0x21);
        put32(zip, e.crc); put32(zip, (uint32_t) e.body.size()); put32(zip, (uint32_t) e.body.size());
        put16(zip, (uint16_t) e.name.size()); put16(zip, 0);
        zip += e.name;
        zip += e.body;
        put32(central, 0x02014b50u); put16(central, 20); put16(central, 20); put16(central, 0); put16(central, 0); put16(central, 0); put16(central, 0x21);
        put32(central, e.crc); put32(central, (uint32_t) e.body.size()); put32(central, (uint32_t) e.body.size());
        put16(central, (uint16_t) e.name.size()); put16(central, 0); put16(central, 0); put16(central, 0); put16(central, 0); put32(central, 0);
        put32(central, e.offset);
        central += e.name;
    }
    const uint32_t cdOffset = (uint32_t) zip.size();
    zip += central;
    put32(zip, 0x06054b50u); put16(zip, 0); put16(zip, 0); put16(zip, (uint16_t) entries.size()); put16(zip, (uint16_t) entries.size());
    put32(zip, (uint32_t) central.size()); put32(zip, cdOffset); put16(zip, 0);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out || std::fwrite(zip.data(), 1, zip.size(), out) != zip.size() || std::fclose(out)) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::printf("%d matrices, Eigen %d.%d.%d -> %s\n", n, version[0], version[1], version[2], argv[2]);
    return 0;
}
