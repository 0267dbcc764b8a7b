// rimphony_tab_install.hip -- a 2-D table set installed from device memory (rimphony_ctx_set_tables_2d_device; gfx950 only):
// the check that every value of ln n is finite, and the three families of spline sweeps that fill the node data of the set
// (tab_install.h has the arithmetic and says why its bits are the host's).  Plain launches, not the persistent kernels: one
// lane solves one line, a grid-stride loop spreads the lines of all tables over the grid, every index is a size_t.  A line is
// a chain of n dependent divisions, so the work is latency-bound and wants many lines in flight, not wide blocks: blocks of
// one wave, as many as there are waves of lines.  The lanes of a wave hold neighbouring mu columns in families 0 and 2 (their
// loads of ln n share cache lines; their stores are 32 bytes apart) and neighbouring gamma rows in family 1 (each lane walks
// its own contiguous row).  The ends of the spline, natural or not-a-knot per axis, travel in the axes of the set
// (RimTabAxis::ends) and are uniform over a launch: the two forms of a line's first and last step do not diverge.
#include <hip/hip_runtime.h>
#include "detmath.h"
#include "tab_install.h"
#include "tab_launch.h"

#define RIM_TAB_INSTALL_BLOCK 64
#define RIM_TAB_INSTALL_MAX_GRID 65536u

// *flag = 1 where any of the `count` values is not finite; the caller has zeroed it
__global__ __launch_bounds__(256) void tab_install_finite_kernel(const double *v, size_t count, unsigned *flag)
{
    const size_t step = (size_t) gridDim.x * blockDim.x;
    bool bad = false;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += step)
        if (!rim_isfinite(v[i])) bad = true;
    if (bad) *flag = 1u;
}

__global__ __launch_bounds__(RIM_TAB_INSTALL_BLOCK) void tab_install_family_kernel(RimTabInstall s, int family)
{
    const size_t lines = rim_tab_install_lines(s, family);
    const size_t step = (size_t) gridDim.x * blockDim.x;
    for (size_t line = (size_t) blockIdx.x * blockDim.x + threadIdx.x; line < lines; line += step)
        rim_tab_install_family_line(s, family, line);
}

static unsigned grid_for(size_t items, unsigned block)
{
    const size_t g = (items + block - 1) / block;
    return g > RIM_TAB_INSTALL_MAX_GRID ? RIM_TAB_INSTALL_MAX_GRID : (unsigned) (g ? g : 1);
}

void rim_tab_install_launch_finite(hipStream_t st, const double *d_log_n, size_t count, unsigned *d_flag)
{
    hipLaunchKernelGGL(tab_install_finite_kernel, dim3(grid_for(count, 256 * 4)), dim3(256), 0, st, d_log_n, count, d_flag);
}

// the three families in order on one stream: family 2 reads what family 1 wrote
void rim_tab_install_launch_sweeps(hipStream_t st, const RimTabInstall &s)
{
    for (int family = 0; family < 3; family++)
        hipLaunchKernelGGL(tab_install_family_kernel, dim3(grid_for(rim_tab_install_lines(s, family), RIM_TAB_INSTALL_BLOCK)),
                           dim3(RIM_TAB_INSTALL_BLOCK), 0, st, s, family);
}
