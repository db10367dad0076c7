// Stand-alone driver of csrc/pmg_symbolic.h, the host part of dxo_pmg_create, for AddressSanitizer and UBSan
// (tests/test_pmg_symbolic_asan.py): the transfer of a chain of quadratic elements (vertices at the even nodes, a midpoint between two
// vertices with the weights 1/2, 1/2), checked, tabulated with a clamped end and compared with the tables written down by hand; then
// every malformed variant of the transfer with its error code. No HIP, no device.
#include "pmg_symbolic.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <utility>
#include <vector>

namespace {

struct Chain {
    std::vector<int64_t> ptr;
    std::vector<int32_t> col, ctf;
    std::vector<double> w;
    int64_t n = 0, nc = 0;
    explicit Chain(int elements) {
        n = 2 * elements + 1, nc = elements + 1;
        ptr.push_back(0);
        for (int64_t i = 0; i < n; ++i) {
            if (i % 2 == 0) {
                col.push_back((int32_t)(i / 2)), w.push_back(1.0);
            } else {
                col.push_back((int32_t)(i / 2)), w.push_back(0.5);
                col.push_back((int32_t)(i / 2 + 1)), w.push_back(0.5);
            }
            ptr.push_back((int64_t)col.size());
        }
        for (int64_t v = 0; v < nc; ++v) ctf.push_back((int32_t)(2 * v));
    }
    dxo_amg_transfer desc() const { return dxo_amg_transfer{nc, ptr.data(), col.data(), w.data(), ctf.data()}; }
};

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

int code_of(const Chain& c, int64_t n) {
    const char* what = nullptr;
    const dxo_amg_transfer d = c.desc();
    const int code = pmg_check_transfer(n, d, &what);
    expect((code == DXO_OK) == (what == nullptr), "a message comes with every error and only with one");
    return code;
}

}  // namespace

int main() {
    for (int elements : {1, 2, 7, 64}) {
        for (int bs : {1, 2, 3}) {
            const Chain c(elements);
            expect(code_of(c, c.n) == DXO_OK, "the chain is a valid transfer");
            // node 0 clamped in every component, the last node in its first component alone
            std::vector<uint8_t> mask((size_t)(c.n * bs), 0);
            for (int k = 0; k < bs; ++k) mask[(size_t)k] = 1;
            mask[(size_t)((c.n - 1) * bs)] = 1;
            pmg_tables t;
            const dxo_amg_transfer d = c.desc();
            pmg_build_tables(c.n, bs, d, mask, t);
            const int64_t pb = c.ptr[(size_t)c.n];
            expect((int64_t)t.p_diag.size() == pb * bs && (int64_t)t.pt_blk.size() == pb && (int64_t)t.pt_row.size() == pb, "sizes");
            expect(t.pt_ptr.front() == 0 && t.pt_ptr.back() == pb && (int64_t)t.pt_ptr.size() == c.nc + 1, "pt_ptr spans the blocks");
            // coarse node v: its own node 2 v, the midpoints 2 v - 1 and 2 v + 1 where they exist, ascending
            for (int64_t v = 0; v < c.nc; ++v) {
                std::vector<int32_t> want;
                if (v > 0) want.push_back((int32_t)(2 * v - 1));
                want.push_back((int32_t)(2 * v));
                if (v + 1 < c.nc) want.push_back((int32_t)(2 * v + 1));
                const int64_t a = t.pt_ptr[(size_t)v], b = t.pt_ptr[(size_t)v + 1];
                expect(b - a == (int64_t)want.size(), "blocks per coarse node");
                for (int64_t e = a; e < b && e - a < (int64_t)want.size(); ++e) {
                    expect(t.pt_row[(size_t)e] == want[(size_t)(e - a)], "fine nodes of a coarse node ascend");
                    const int64_t blk = t.pt_blk[(size_t)e];
                    expect(blk >= c.ptr[(size_t)t.pt_row[(size_t)e]] && blk < c.ptr[(size_t)t.pt_row[(size_t)e] + 1] && c.col[(size_t)blk] == v,
                           "a block of the incidence is the block (fine node, coarse node)");
                }
            }
            // p_diag: the weight, zero where the fine dof or the coarse node's dof is clamped
            for (int64_t i = 0; i < c.n; ++i)
                for (int64_t e = c.ptr[(size_t)i]; e < c.ptr[(size_t)i + 1]; ++e)
                    for (int k = 0; k < bs; ++k) {
                        const int64_t f = c.ctf[(size_t)c.col[(size_t)e]];
                        const bool off = mask[(size_t)(i * bs + k)] || mask[(size_t)(f * bs + k)];
                        expect(t.p_diag[(size_t)(e * bs + k)] == (off ? 0.0 : c.w[(size_t)e]), "p_diag");
                    }
            // the coarse constrained list: node 0 entirely, the last coarse node in its first component
            std::vector<int32_t> want;
            for (int k = 0; k < bs; ++k) want.push_back((int32_t)k);
            want.push_back((int32_t)((c.nc - 1) * bs));
            expect(t.c_bc == want, "coarse constrained dofs");
        }
    }
    // the malformed transfers
    const Chain good(4);
    {
        Chain c = good;
        c.nc = 0;
        expect(code_of(c, c.n) == DXO_E_SIZE, "n_coarse < 1");
        c.nc = good.n + 1;
        expect(code_of(c, c.n) == DXO_E_SIZE, "n_coarse > n_nodes");
    }
    {
        Chain c = good;
        c.ptr[0] = 1;
        expect(code_of(c, c.n) == DXO_E_SIZE, "ptr[0] != 0");
    }
    {
        Chain c = good;
        c.ptr[2] = c.ptr[1];
        expect(code_of(c, c.n) == DXO_E_SIZE, "a node without an entry");
    }
    {
        Chain c = good;
        c.col[2] = (int32_t)c.nc;
        expect(code_of(c, c.n) == DXO_E_SIZE, "a column beyond the range");
        c.col[2] = -1;
        expect(code_of(c, c.n) == DXO_E_SIZE, "a negative column");
    }
    {
        Chain c = good;
        std::swap(c.col[1], c.col[2]);
        expect(code_of(c, c.n) == DXO_E_OPTION, "columns not ascending");
    }
    {
        Chain c = good;
        c.w[1] = std::numeric_limits<double>::quiet_NaN();
        expect(code_of(c, c.n) == DXO_E_OPTION, "a weight that is not finite");
        c.w[1] = std::numeric_limits<double>::infinity();
        expect(code_of(c, c.n) == DXO_E_OPTION, "an infinite weight");
    }
    {
        Chain c = good;
        c.ctf[1] = c.ctf[0];
        expect(code_of(c, c.n) == DXO_E_OPTION, "coarse_to_fine names a node twice");
        c.ctf[1] = (int32_t)c.n;
        expect(code_of(c, c.n) == DXO_E_SIZE, "coarse_to_fine beyond the range");
        c.ctf[1] = -1;
        expect(code_of(c, c.n) == DXO_E_SIZE, "coarse_to_fine negative");
        c.ctf[1] = 1;
        expect(code_of(c, c.n) == DXO_E_OPTION, "the row of coarse_to_fine[v] has two entries");
    }
    {
        Chain c = good;
        c.w[0] = 0.5;
        expect(code_of(c, c.n) == DXO_E_OPTION, "the row of coarse_to_fine[v] has another weight than 1");
    }
    if (failures) return 1;
    std::printf("pmg symbolic harness: ok\n");
    return 0;
}
