// mesh_table.h — the 6 x 16 triangle table of marching tetrahedra on Kuhn's split of a cube, generated at compile time.
//
// Corner code of a cell corner: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Tetrahedron k is the path 0 -> e_p1 -> e_p1 + e_p2 -> (1,1,1) for the
// k-th permutation p of the axes in lexicographic order; a case is the 4 inside bits of the path's corners (bit i = path corner i).
// Every edge of a Kuhn tetrahedron joins two comparable corners, so its lower end -- the lattice vertex that owns it -- is the AND of the
// two corner codes, and the slot is a function of their XOR.  A table entry packs the three edges of a triangle, 6 bits each:
// bits 0-2 the owner's corner code, bits 3-5 the slot.
// Orientation (include/sanerf_hip.h): a triangle's last two vertices are swapped where the normal of its edge mid-points on the unit lattice
// points from the outside corners' centroid to the inside corners'; integers throughout, and `bad` records a zero dot product.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define SN_TABLE_FN __host__ __device__ constexpr
#else
#define SN_TABLE_FN constexpr
#endif

namespace sn {

struct TetTable {
    uint32_t tri[6][16][2];
    bool bad;
};

// slot e of a lattice vertex goes to the neighbour at offset (1,0,0),(0,1,0),(0,0,1),(1,1,0),(1,0,1),(0,1,1),(1,1,1): as corner codes
SN_TABLE_FN uint32_t slot_corner(int e) { return (0x7653421u >> (4 * e)) & 7u; }
// ... and back: the slot of an offset's corner code (1 .. 7)
SN_TABLE_FN uint32_t corner_slot(uint32_t code) { return (0x65423100u >> (4 * code)) & 7u; }

SN_TABLE_FN int tet_axis(int k, int i) {              // axis i of the k-th permutation of (0,1,2), lexicographic
    const int first = k / 2;
    if (i == 0) return first;
    const int lo = first == 0 ? 1 : 0, hi = first == 2 ? 1 : 2;          // the two other axes, ascending
    const bool ascending = (k % 2) == 0;
    if (i == 1) return ascending ? lo : hi;
    return ascending ? hi : lo;
}

SN_TABLE_FN uint32_t tet_corner(int k, int i) {        // corner code of path corner i of tetrahedron k
    if (i == 0) return 0u;
    if (i == 1) return 1u << tet_axis(k, 0);
    if (i == 2) return (1u << tet_axis(k, 0)) | (1u << tet_axis(k, 1));
    return 7u;
}

constexpr TetTable make_tet_table() {
    TetTable T{};
    for (int k = 0; k < 6; ++k) {
        for (int cs = 0; cs < 16; ++cs) {
            int I[4] = {0, 0, 0, 0}, O[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int i = 0; i < 4; ++i) {
                if ((cs >> i) & 1) I[ni++] = i;
                else O[no++] = i;
            }
            int tr[2][3][2] = {};
            int nt = 0;
            if (ni == 1) {
                for (int q = 0; q < 3; ++q) { tr[0][q][0] = I[0]; tr[0][q][1] = O[q]; }
                nt = 1;
            } else if (ni == 3) {
                for (int q = 0; q < 3; ++q) { tr[0][q][0] = I[q]; tr[0][q][1] = O[0]; }
                nt = 1;
            } else if (ni == 2) {
                const int a[2] = {I[0], O[0]}, b[2] = {I[0], O[1]}, c[2] = {I[1], O[1]}, d[2] = {I[1], O[0]};
                for (int s = 0; s < 2; ++s) {
                    tr[0][0][s] = a[s]; tr[0][1][s] = b[s]; tr[0][2][s] = c[s];
                    tr[1][0][s] = a[s]; tr[1][1][s] = c[s]; tr[1][2][s] = d[s];
                }
                nt = 2;
            }
            for (int j = 0; j < nt; ++j) {
                int m[3][3] = {};
                for (int q = 0; q < 3; ++q)
                    for (int ax = 0; ax < 3; ++ax)
                        m[q][ax] = (int)((tet_corner(k, tr[j][q][0]) >> ax) & 1u) + (int)((tet_corner(k, tr[j][q][1]) >> ax) & 1u);
                int u[3] = {}, w[3] = {}, din[3] = {}, dout[3] = {};
                for (int ax = 0; ax < 3; ++ax) { u[ax] = m[1][ax] - m[0][ax]; w[ax] = m[2][ax] - m[0][ax]; }
                const int n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
                for (int ax = 0; ax < 3; ++ax) {
                    for (int i = 0; i < ni; ++i) din[ax] += (int)((tet_corner(k, I[i]) >> ax) & 1u);
                    for (int i = 0; i < no; ++i) dout[ax] += (int)((tet_corner(k, O[i]) >> ax) & 1u);
                }
                int dot = 0;
                for (int ax = 0; ax < 3; ++ax) dot += n[ax] * (dout[ax] * ni - din[ax] * no);
                if (dot == 0) T.bad = true;
                const int order[3] = {0, dot > 0 ? 1 : 2, dot > 0 ? 2 : 1};
                uint32_t packed = 0u;
                for (int q = 0; q < 3; ++q) {
                    const uint32_t cp = tet_corner(k, tr[j][order[q]][0]), cq = tet_corner(k, tr[j][order[q]][1]);
                    packed |= ((cp & cq) | (corner_slot(cp ^ cq) << 3)) << (6 * q);
                }
                T.tri[k][cs][j] = packed;
            }
        }
    }
    return T;
}

}  // namespace sn
