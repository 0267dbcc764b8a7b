// rimphony_tab_group.hip -- group_kernel<P> (group_kernel.h) for the tabulated distribution (RIMPHONY_TABULATED; gfx950 only):
// the Symphony coefficients of a parameter point in lock-step, one instantiation per form of the installed table set.  In a
// group the table lookup of a sample -- the cubic of the energy table, the pitch row's, the bicubic of a 2-D set, the pow of
// a sin^k prefactor -- is evaluated once for all members that need it (dev_symphony.h: gamma_integrand_f_terms calls
// calc_f_both once), where one wave per coefficient evaluates it for every member again.
//
// A translation unit of its own: hipcc's code generation for a kernel of this size depends on what else is in the unit
// (rimphony_internal.h), so these four must not move the four of rimphony_group.hip.  Nor must the fifth, of a set on given
// gamma nodes, move these: it is rimphony_tab_grid_group.hip's, reached through the one lookup here, and the sixth, of a 2-D
// set on given nodes, is rimphony_tab_2d_grid_group.hip's; those of the 2-D forms with a sin^k prefactor are
// rimphony_tab_2d_pitchy_group.hip's and rimphony_tab_2d_grid_pitchy_group.hip's, those of the 2-D form on given gamma and mu
// nodes rimphony_tab_2d_nodes_group.hip's and rimphony_tab_2d_nodes_pitchy_group.hip's, those of the families of energy tables
// rimphony_tab_family_group.hip's and rimphony_tab_family_pitchy_group.hip's, those of the families of 2-D surfaces
// rimphony_tab_2d_family_group.hip's and rimphony_tab_2d_family_pitchy_group.hip's, those of the same families blended
// cubically rimphony_tab_2d_family_cubic_group.hip's and rimphony_tab_2d_family_cubic_pitchy_group.hip's.  They live with the
// budget of rimphony_group.hip's: RIM_GROUP_WAVES waves per SIMD and the same LDS block.  The kind has no Faraday group
// (RIMPHONY_FARADAY_GROUP is measured slower for the analytic kinds: DESIGN.md section 5).
#include "group_kernel.h"
#include "tab_launch.h"

const void *rim_tab_group_kernel(int tab_kind)
{
    return rim_with_tab_kind(tab_kind, [](auto K) {
        constexpr int KIND = decltype(K)::value;
        if constexpr (KIND == DIST_TABULATED_GRID) return rim_tab_grid_group_kernel();     // not in this unit: see above
        else if constexpr (KIND == DIST_TABULATED_2D_GRID) return rim_tab_2d_grid_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_2D_PITCHY) return rim_tab_2d_pitchy_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_2D_GRID_PITCHY) return rim_tab_2d_grid_pitchy_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_2D_NODES) return rim_tab_2d_nodes_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_2D_NODES_PITCHY) return rim_tab_2d_nodes_pitchy_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_FAMILY) return rim_tab_family_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_FAMILY_PITCHY) return rim_tab_family_pitchy_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY) return rim_tab_2d_family_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_PITCHY) return rim_tab_2d_family_pitchy_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC) return rim_tab_2d_family_cubic_group_kernel();
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY) return rim_tab_2d_family_cubic_pitchy_group_kernel();
        else return reinterpret_cast<const void *>(group_kernel<SymGroupProblem<KIND>>);
    });
}
