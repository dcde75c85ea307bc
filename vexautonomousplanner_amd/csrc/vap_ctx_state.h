// vap_ctx_state.h — the readers of vap_ctx::left, the record of the batch the last sampling or profile call left on the
// context (vap_internal.h; DESIGN.md section 1, "What a call leaves on the context").  An entry point that takes NULL
// for "the context's own" asks here, with the shape it was called with, and gets the pointers or the refusal.
#pragma once
#include "vap_internal.h"
#include "vap_kernels.h"

struct VapTables {
    const double *seg = nullptr, *lut = nullptr;
    vap::RouteTables rt;    // of a batch of routes cut into splines (rt.sptab set), else the defaults of plain paths
};

// The tables of a B x W batch: VAP_ERR_UNFITTED without them; plain_only callers refuse those of split routes.
inline int vap_ctx_tables(const vap_ctx *ctx, int B, int W, bool plain_only, VapTables &t)
{
    const VapLeft &l = ctx->left;
    if (l.tab_B != B || l.tab_W != W || !ctx->seg.ptr || !ctx->lut.ptr)
        return vap_fail(VAP_ERR_UNFITTED, "no tables of a %d x %d batch in this context (last profile call: %d x %d)", B, W, l.tab_B,
                        l.tab_W);
    if (plain_only && l.routes())
        return vap_fail(VAP_ERR_UNSUPPORTED, "the batch on the context is one of split routes (vap_profile_routes): their "
                                             "time domain goes through vap_time_profile_routes / vap_time_insert_events");
    t.seg = (const double *)ctx->seg.ptr;
    t.lut = (const double *)ctx->lut.ptr;
    if (l.routes()) t.rt = vap::RouteTables{(const double *)ctx->sptab.ptr, (const int *)ctx->nspl.ptr, l.NS};
    return VAP_OK;
}

// The distance grid of a B x W x S batch.
inline int vap_ctx_grid(const vap_ctx *ctx, int B, int W, int S, const double *&aux, const double *&runs)
{
    const VapLeft &l = ctx->left;
    if (l.B != B || l.W != W || l.S != S || !ctx->runs.ptr || !ctx->aux.ptr)
        return vap_fail(VAP_ERR_INVALID, "no distance grid of this shape on the context (%d x %d x %d; the last sampling call left %d x %d x %d)",
                        B, W, S, l.B, l.W, l.S);
    aux = (const double *)ctx->aux.ptr;
    runs = (const double *)ctx->runs.ptr;
    return VAP_OK;
}

// The rows for a velocity pass of B x S in dtype dt with d_dtheta == NULL.  VAP_F32 with the fp64 recurrence: both rows
// come from the context, in fp64 (r64 is set); otherwise the |dtheta| rows only, and the curvature stays the caller's.
inline int vap_ctx_rows(const vap_ctx *ctx, vap_dtype dt, int B, int S, const void *&curvature, const void *&dtheta, bool &r64)
{
    const VapLeft &l = ctx->left;
    if (l.rows == VAP_ROWS_NONE || l.B != B || l.S != S || l.rows_dt != (int)dt)
        return vap_fail(VAP_ERR_INVALID, "d_dtheta is NULL and the context holds no rows of this shape and dtype (%d x %d, dtype %d; "
                        "the last sampling call left %s %d x %d, dtype %d)", B, S, (int)dt, l.rows != VAP_ROWS_NONE ? "rows of" : "no rows;",
                        l.B, l.S, l.rows_dt);
    if (l.rows == VAP_ROWS_HI) {
        curvature = ctx->k64.ptr;
        dtheta = ctx->dth64.ptr;
        r64 = true;
    } else {
        dtheta = ctx->dth.ptr;
    }
    return VAP_OK;
}

// A time-domain entry point integrates the caller's velocity row as it is now — plus, for an fp32 row whose velocity pass
// ran the fp64 recurrence in this context, the fp32 residual that pass left behind, returned here (row + residual = the
// fp64 velocity to 2^-48; MPG:566-584 integrates positions from the row, and an fp32 row alone moves a position by ~1e-7
// relative, now and then across a boundary of the reference's step lookup, SM:550-580).  The residual is below the
// row's own rounding, so a row the caller has edited since is integrated as edited.  Null: no residual for this row.
inline const float *vap_ctx_residual(const vap_ctx *ctx, vap_dtype dt, int B, int S, const void *d_velocity)
{
    const VapLeft &l = ctx->left;
    if (dt == VAP_F32 && l.vres_for == d_velocity && ctx->vres.ptr && l.vres_B == B && l.vres_S == S) return (const float *)ctx->vres.ptr;
    return nullptr;
}
