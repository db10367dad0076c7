// Host-only harness for tests/test_functional_host_asan.py: the argument checks of csrc/functional.hip (everything its entry points do
// before the first HIP call) under AddressSanitizer + UBSan, on the CPU. The context, mesh and facet sets are plain structs filled in
// by hand; no call below gets as far as a device: each must return its code first. Built as host code only (no kernel is compiled or
// launched) and linked against libdxo_hip.so for the symbols of the other translation units.
#include <cstdio>
#include <cstring>

#include "dxo_common.h"
#include "facet_tabs.h"

static int failures = 0;

static void expect(dxo_ctx* ctx, int rc, int code, const char* who, const char* what) {
    const bool named = code == DXO_OK || std::strstr(ctx->err.c_str(), who) != nullptr;
    if (rc != code || !named) {
        std::printf("FAIL %s (%s): rc %d, expected %d, last error '%s'\n", who, what, rc, code, ctx->err.c_str());
        ++failures;
    }
    ctx->err.clear();
}

int main() {
    dxo_ctx ctx;
    dxo_mesh mesh, other;
    for (dxo_mesh* m : {&mesh, &other}) {
        m->gdim = 2;
        m->num_cells = 4;
        m->num_field_nodes = m->num_geom_nodes = 9;
        m->dev.nq = 3;
        m->dev.ndofs = m->dev.ngeom = 3;
        m->dev.cells_per_wave = 21;
        m->dev.wave_doubles = 384;
        m->dev.table_doubles = 64;
    }
    alignas(16) static double buf[256];
    alignas(16) static int32_t cells[8] = {0, 1, 2, 3, 0, 1, 2, 3};
    double* odd = reinterpret_cast<double*>(reinterpret_cast<char*>(buf) + 4);
    const int32_t* odd_cells = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(cells) + 2);

    // weights not set
    expect(&ctx, dxo_eval_cell_measure(&ctx, &mesh, nullptr, 4, buf), DXO_E_OPTION, "dxo_eval_cell_measure", "no weights");
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, 3, buf, nullptr, buf), DXO_E_OPTION, "dxo_integrate", "no weights");
    expect(&ctx, dxo_operand_moments(&ctx, &mesh, DXO_OPERAND_VALUE, 1, buf, nullptr, 4, buf), DXO_E_OPTION, "dxo_operand_moments", "no weights");
    mesh.d_wq = other.d_wq = buf;

    // NULL context, mesh, arrays
    if (dxo_integrate(nullptr, &mesh, nullptr, 4, 3, buf, nullptr, buf) != DXO_E_NULL) ++failures;
    expect(&ctx, dxo_eval_cell_measure(&ctx, nullptr, nullptr, 4, buf), DXO_E_NULL, "dxo_eval_cell_measure", "mesh NULL");
    expect(&ctx, dxo_eval_cell_measure(&ctx, &mesh, nullptr, 4, nullptr), DXO_E_NULL, "dxo_eval_cell_measure", "dx NULL");
    expect(&ctx, dxo_eval_cell_measure(&ctx, &mesh, nullptr, 0, nullptr), DXO_OK, "dxo_eval_cell_measure", "nothing to do");
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, 3, nullptr, nullptr, buf), DXO_E_NULL, "dxo_integrate", "f NULL");
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, 3, buf, nullptr, nullptr), DXO_E_NULL, "dxo_integrate", "out NULL");
    expect(&ctx, dxo_integrate(&ctx, &mesh, cells, 0, 3, nullptr, nullptr, nullptr), DXO_E_NULL, "dxo_integrate", "out NULL, empty list");
    expect(&ctx, dxo_operand_moments(&ctx, &mesh, DXO_OPERAND_VALUE, 1, nullptr, nullptr, 4, buf), DXO_E_NULL, "dxo_operand_moments", "u NULL");
    expect(&ctx, dxo_operand_moments(&ctx, &mesh, DXO_OPERAND_VALUE, 1, buf, nullptr, 4, nullptr), DXO_E_NULL, "dxo_operand_moments", "out NULL");

    // sizes
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 5, 3, buf, nullptr, buf), DXO_E_SIZE, "dxo_integrate", "more cells than the mesh has");
    expect(&ctx, dxo_integrate(&ctx, &mesh, cells, -1, 3, buf, nullptr, buf), DXO_E_SIZE, "dxo_integrate", "negative list length");

    // misalignment
    expect(&ctx, dxo_eval_cell_measure(&ctx, &mesh, nullptr, 4, odd), DXO_E_ALIGN, "dxo_eval_cell_measure", "dx");
    expect(&ctx, dxo_eval_cell_measure(&ctx, &mesh, odd_cells, 4, buf), DXO_E_ALIGN, "dxo_eval_cell_measure", "cells");
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, 3, odd, nullptr, buf), DXO_E_ALIGN, "dxo_integrate", "f");
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, 3, buf, odd, buf), DXO_E_ALIGN, "dxo_integrate", "g");
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, 3, buf, nullptr, odd), DXO_E_ALIGN, "dxo_integrate", "out");
    expect(&ctx, dxo_operand_moments(&ctx, &mesh, DXO_OPERAND_VALUE, 1, odd, nullptr, 4, buf), DXO_E_ALIGN, "dxo_operand_moments", "u");

    // D outside the served set; the pairing's range
    for (int D : {0, -3, 5, 7, 8, 10, 1 << 30})
        expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, D, buf, nullptr, buf), DXO_E_DIM, "dxo_integrate", "D not served");
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, 0, buf, buf, buf), DXO_E_DIM, "dxo_integrate", "pairing, D = 0");
    expect(&ctx, dxo_integrate(&ctx, &mesh, nullptr, 4, (1 << 24) + 1, buf, buf, buf), DXO_E_DIM, "dxo_integrate", "pairing, D above 2^24");

    // kinds and block sizes of the fused form
    expect(&ctx, dxo_operand_moments(&ctx, &mesh, 99, 1, buf, nullptr, 4, buf), DXO_E_OPTION, "dxo_operand_moments", "unknown kind");
    expect(&ctx, dxo_operand_moments(&ctx, &mesh, DXO_OPERAND_VALUE, 5, buf, nullptr, 4, buf), DXO_E_DIM, "dxo_operand_moments", "bs without a fused form");
    expect(&ctx, dxo_operand_moments(&ctx, &mesh, DXO_OPERAND_EPS_MANDEL, 1, buf, nullptr, 4, buf), DXO_E_DIM, "dxo_operand_moments", "eps of a scalar");
    expect(&ctx, dxo_operand_moments(&ctx, &mesh, DXO_OPERAND_DETF, 3, buf, nullptr, 4, buf), DXO_E_DIM, "dxo_operand_moments", "bs = 3 on gdim 2");

    // the facet call: NULL set, tables / geometry not set, a foreign set, a changed (nf, nq), then arrays
    dxo_facet_set set, foreign;
    set.mesh = &mesh;
    foreign.mesh = &other;
    set.n = foreign.n = 2;
    set.nf = foreign.nf = 3;
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, nullptr, 1, buf, nullptr, buf), DXO_E_NULL, "dxo_facet_integrate", "set NULL");
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &set, 1, buf, nullptr, buf), DXO_E_OPTION, "dxo_facet_integrate", "no facet tables");
    mesh.d_facet_tab = buf;
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &set, 1, buf, nullptr, buf), DXO_E_OPTION, "dxo_facet_integrate", "no facet geometry");
    mesh.d_facet_geom = buf;
    mesh.n_local_facets = mesh.nf_geom = 3;
    mesh.nq_facet = mesh.nq_geom = 2;
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &foreign, 1, buf, nullptr, buf), DXO_E_DIM, "dxo_facet_integrate", "foreign set");
    mesh.nq_geom = 3;
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &set, 1, buf, nullptr, buf), DXO_E_DIM, "dxo_facet_integrate", "geometry of another rule");
    mesh.nq_geom = 2;
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &set, 5, buf, nullptr, buf), DXO_E_DIM, "dxo_facet_integrate", "D not served");
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &set, 1, nullptr, nullptr, buf), DXO_E_NULL, "dxo_facet_integrate", "f NULL");
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &set, 1, buf, nullptr, nullptr), DXO_E_NULL, "dxo_facet_integrate", "out NULL");
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &set, 1, odd, nullptr, buf), DXO_E_ALIGN, "dxo_facet_integrate", "f");
    expect(&ctx, dxo_facet_integrate(&ctx, &mesh, &set, 1, buf, odd, buf), DXO_E_ALIGN, "dxo_facet_integrate", "g");

    if (failures) {
        std::printf("functional argument harness: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("functional argument harness: ok\n");
    return 0;
}
