// vap_plan.h — the planner's grid, shared by vap_plan.hip (clearance grid, seeds) and vap_occupancy.hip (routes rasterised
// onto the same grid).  Definitions: include/vap.h.
#pragma once
#include "vap_footprint.h"

namespace vap {

constexpr int kPlanMaxCells = 16384;

struct PlanGrid {
    double xmin, ymin, xmax, ymax, cell;
    int nx, ny;
};

__device__ __forceinline__ double plan_centre(double lo, int i, double cell) { return lo + ((double)i + 0.5) * cell; }

// The grid of a validated field box over `cell` (include/vap.h: nx = ceil((xmax - xmin) / cell), at most kPlanMaxCells
// cells).  Host only; defined in vap_plan.hip.
int plan_grid_of(const double *h_field, double cell, PlanGrid &g);

}  // namespace vap
