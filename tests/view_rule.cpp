// The rule of csrc/trs_view.h on plain host arrays: whatever nJ, nM, n_free, the end joints, joint_out and free_index
// hold, TrsBatch::truss(b) trims every count to the arrays and hands out no index outside them.  Every array is a
// heap allocation of exactly its size, so a build with -fsanitize=address,undefined sees any read outside one.
// Exit status 0 and "view rule ok" when every check holds.
#include <cstdio>
#include <vector>

#include "trs_view.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);   \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Arrays {
    int B, nJ_max, nM_max, ld_f;
    std::vector<double> xyz, E, A, types;
    std::vector<int> conn, free_index, n_free, nJ, nM, joint_out;
    std::vector<unsigned short> conn16;
    std::vector<unsigned char> tidx;
    Arrays(int B_, int nJ_max_, int nM_max_, int ld_f_)
        : B(B_), nJ_max(nJ_max_), nM_max(nM_max_), ld_f(ld_f_), xyz((size_t)B_ * 3 * nJ_max_, 1.0),
          E((size_t)B_ * nM_max_, 2.0), A((size_t)B_ * nM_max_, 3.0), types(3, 1.0), conn((size_t)B_ * nM_max_ * 2, 0),
          free_index((size_t)B_ * 3 * nJ_max_, -1), n_free(B_, 0), nJ(B_, 0), nM(B_, 0),
          joint_out((size_t)B_ * nJ_max_, 0), conn16((size_t)B_ * nM_max_ * 2, 0), tidx((size_t)B_ * nM_max_, 0) {}
    TrsBatch general(bool with_order = true) const {
        return trs_batch(nJ_max, nM_max, xyz.data(), trs_members_general(conn.data(), E.data(), A.data()),
                         free_index.data(), n_free.data(), nJ.data(), nM.data(), with_order ? joint_out.data() : nullptr,
                         ld_f);
    }
    TrsBatch table() const {
        return trs_batch(nJ_max, nM_max, xyz.data(), trs_members_table(conn16.data(), tidx.data(), types.data()),
                         free_index.data(), n_free.data(), nJ.data(), nM.data(), joint_out.data(), ld_f);
    }
};

// what must hold of ANY truss of ANY batch: trimmed counts, every index inside its array
static void check_inside(const TrsBatch& bt, int b) {
    const TrussView v = bt.truss(b);
    CHECK(v.joints >= 0 && v.joints <= bt.nJ_max);
    CHECK(v.members >= 0 && v.members <= bt.nM_max);
    CHECK(bt.nJ_max > 0 || v.members == 0);
    CHECK(v.nfree >= 0 && v.nfree <= bt.ld_f);
    CHECK(v.ndof == 3 * v.joints && v.ndof_max == 3 * bt.nJ_max);
    CHECK(v.fi == bt.free_index + (size_t)b * 3 * bt.nJ_max);
    CHECK(v.X == (bt.xyz != nullptr ? bt.xyz + (size_t)b * 3 * bt.nJ_max : nullptr));
    CHECK(v.mbase == (size_t)b * bt.nM_max);
    for (int d = 0; d < v.ndof_max + 2; ++d) {   // (a DOF is a loop index or 3 j + a of a clamped joint: never negative)
        const int r = v.row_of(d);
        CHECK(r >= -1 && r < v.nfree);
        if (d >= v.ndof) CHECK(r == -1);   // past the truss's own joints
    }
    for (int j = 0; j < bt.nJ_max; ++j) {
        const int id = v.place(j);
        CHECK(id >= 0 && id < bt.nJ_max);
        const int raw = v.jo != nullptr ? v.jo[j] : j;
        CHECK(id == ((raw >= 0 && raw < bt.nJ_max) ? raw : j));   // the fallback
        const int o = v.place_dof(3 * j + 2);
        CHECK(o == 3 * id + 2);
        const TrussView::Rows rows = v.rows(j);
        for (int a = 0; a < 3; ++a) {
            CHECK(rows.r[a] == v.row_of(3 * j + a));
            CHECK(v.held(j, a) == (rows.r[a] < 0) && rows.held(a) == v.held(j, a));
        }
        CHECK(rows.any_held() == (v.held(j, 0) || v.held(j, 1) || v.held(j, 2)) && v.any_held(j) == rows.any_held());
        CHECK(rows.all_held() == (v.held(j, 0) && v.held(j, 1) && v.held(j, 2)) && v.all_held(j) == rows.all_held());
    }
    for (int m = 0; m < v.members; ++m) {
        const TrussView::Ends e = v.ends(m);
        const int2 raw = v.raw_ends(m);
        CHECK(e.c.x >= 0 && e.c.x < bt.nJ_max && e.c.y >= 0 && e.c.y < bt.nJ_max);
        CHECK(e.inside == (raw.x >= 0 && raw.x < v.joints && raw.y >= 0 && raw.y < v.joints));
        if (e.inside) CHECK(e.c.x == raw.x && e.c.y == raw.y);
    }
}

static void well_formed() {
    Arrays h(2, 4, 3, 8);
    const int joints[2] = {3, 4}, members[2] = {2, 3}, rows[2] = {5, 7};
    const int ends[2][3][2] = {{{0, 1}, {1, 2}, {0, 0}}, {{0, 3}, {3, 1}, {2, 1}}};
    const int order[2][4] = {{2, 0, 1, 3}, {3, 2, 1, 0}};
    for (int b = 0; b < 2; ++b) {
        h.nJ[b] = joints[b];
        h.nM[b] = members[b];
        h.n_free[b] = rows[b];
        int next = 0;
        for (int d = 0; d < 3 * joints[b]; ++d) h.free_index[(size_t)b * 12 + d] = (d % 4 == 0 || next >= rows[b]) ? -1 : next++;
        CHECK(next == rows[b]);
        for (int m = 0; m < 3; ++m)
            for (int s = 0; s < 2; ++s) {
                h.conn[((size_t)b * 3 + m) * 2 + s] = ends[b][m][s];
                h.conn16[((size_t)b * 3 + m) * 2 + s] = (unsigned short)ends[b][m][s];
            }
        for (int j = 0; j < 4; ++j) h.joint_out[(size_t)b * 4 + j] = order[b][j];
    }
    const TrsBatch forms[3] = {h.general(), h.table(), h.general(false)};
    for (int f = 0; f < 3; ++f)
        for (int b = 0; b < 2; ++b) {
            check_inside(forms[f], b);
            const TrussView v = forms[f].truss(b);
            // nothing is trimmed, clamped or replaced on well-formed input
            CHECK(v.joints == joints[b] && v.members == members[b] && v.nfree == rows[b]);
            for (int d = 0; d < v.ndof; ++d) CHECK(v.row_of(d) == h.free_index[(size_t)b * 12 + d]);
            for (int j = 0; j < 4; ++j) CHECK(v.place(j) == (f == 2 ? j : order[b][j]));
            for (int m = 0; m < v.members; ++m) {
                const TrussView::Ends e = v.ends(m);
                CHECK(e.inside && e.c.x == ends[b][m][0] && e.c.y == ends[b][m][1]);
            }
            CHECK(v.held(0, 0) && !v.held(0, 1) && v.any_held(0) && !v.all_held(0));
        }
}

static void malformed() {
    // counts negative and past the maxima, end joints of -1 and nJ_max (65535 in the table form), joint_out and
    // free_index entries outside the arrays
    Arrays h(4, 4, 3, 8);
    const int nJ[4] = {-3, 99, 2, 4}, nM[4] = {99, -1, 3, 3}, nf[4] = {-7, 1000, 8, 3};
    for (int b = 0; b < 4; ++b) {
        h.nJ[b] = nJ[b];
        h.nM[b] = nM[b];
        h.n_free[b] = nf[b];
        for (int d = 0; d < 12; ++d) h.free_index[(size_t)b * 12 + d] = d == 1 ? 8 : d == 2 ? 1 << 30 : d == 3 ? -9 : d % 8;
        const int ends[3][2] = {{-1, 1}, {2, 4}, {3, 0}};
        for (int m = 0; m < 3; ++m)
            for (int s = 0; s < 2; ++s) {
                h.conn[((size_t)b * 3 + m) * 2 + s] = ends[m][s];
                h.conn16[((size_t)b * 3 + m) * 2 + s] = ends[m][s] < 0 ? 65535 : (unsigned short)ends[m][s];
            }
        const int order[4] = {-5, 4, 1, 1 << 30};
        for (int j = 0; j < 4; ++j) h.joint_out[(size_t)b * 4 + j] = order[j];
    }
    const TrsBatch forms[2] = {h.general(), h.table()};
    for (int f = 0; f < 2; ++f) {
        for (int b = 0; b < 4; ++b) check_inside(forms[f], b);
        const TrussView v0 = forms[f].truss(0), v1 = forms[f].truss(1), v2 = forms[f].truss(2), v3 = forms[f].truss(3);
        CHECK(v0.joints == 0 && v0.members == 3 && v0.nfree == 0);
        CHECK(v1.joints == 4 && v1.members == 0 && v1.nfree == 8);
        CHECK(v2.joints == 2 && v2.members == 3 && v2.nfree == 8);
        CHECK(v1.row_of(0) == 0 && v1.row_of(1) == -1 && v1.row_of(2) == -1 && v1.row_of(3) == -1 && v1.row_of(7) == 7);
        CHECK(v3.row_of(4) == -1 && v3.row_of(10) == 2);   // a row at or past n_free is held
        CHECK(v2.row_of(5) == 5 && v2.row_of(6) == -1);    // DOF 6 belongs to no joint of this truss
        CHECK(v1.place(0) == 0 && v1.place(1) == 1 && v1.place(2) == 1 && v1.place(3) == 3);
        const TrussView::Ends e0 = v3.ends(0), e1 = v3.ends(1), e2 = v3.ends(2);
        CHECK(!e0.inside && e0.c.x == (f == 0 ? 0 : 3) && e0.c.y == 1);
        CHECK(!e1.inside && e1.c.x == 2 && e1.c.y == 3);
        CHECK(e2.inside && e2.c.x == 3 && e2.c.y == 0);
        CHECK(!v2.ends(2).inside);   // joint 3 is in the arrays, not in this truss of two joints
    }
    // no joints at all: no member either (there is no end to clamp to), every DOF is held
    Arrays z(1, 0, 3, 8);
    z.nJ[0] = 5;
    z.nM[0] = 3;
    z.n_free[0] = 4;
    const TrsBatch none = z.general();
    check_inside(none, 0);
    const TrussView v = none.truss(0);
    CHECK(v.joints == 0 && v.members == 0 && v.ndof == 0 && v.ndof_max == 0 && v.row_of(0) == -1);
    // a batch that leaves a count out: the arrays' own size
    const TrsBatch dofs = trs_batch_dofs(h.nJ_max, h.free_index.data(), nullptr, nullptr, nullptr, h.ld_f);
    const TrussView w = dofs.truss(3);   // (xyz is null here: no X is formed)
    CHECK(w.joints == 4 && w.nfree == 8 && w.members == 0 && w.row_of(4) == 4 && w.place(2) == 2 && w.X == nullptr);
}

int main() {
    well_formed();
    malformed();
    if (failures != 0) {
        std::printf("view rule: %d checks failed\n", failures);
        return 1;
    }
    std::printf("view rule ok\n");
    return 0;
}
