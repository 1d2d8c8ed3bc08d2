/* abi_check.c - compile-time proof that the public structs are laid out like the reference's
 * (x86-64 LP64 offsets recorded in SURVEY.md section 8b against src/pll.h:241-335). The GPU box
 * has no reference header to compare with, so the record lives here as static assertions. */
#include <stddef.h>

#include "pll_internal.h"

#define AT(type, field, off) _Static_assert(offsetof(type, field) == (off), #type "." #field " moved")

_Static_assert(sizeof(pll_partition_t) == 232, "pll_partition_t size");
AT(pll_partition_t, tips, 0);
AT(pll_partition_t, clv_buffers, 4);
AT(pll_partition_t, nodes, 8);
AT(pll_partition_t, states, 12);
AT(pll_partition_t, sites, 16);
AT(pll_partition_t, pattern_weight_sum, 20);
AT(pll_partition_t, rate_matrices, 24);
AT(pll_partition_t, prob_matrices, 28);
AT(pll_partition_t, rate_cats, 32);
AT(pll_partition_t, scale_buffers, 36);
AT(pll_partition_t, attributes, 40);
AT(pll_partition_t, alignment, 48);
AT(pll_partition_t, states_padded, 56);
AT(pll_partition_t, clv, 64);
AT(pll_partition_t, pmatrix, 72);
AT(pll_partition_t, rates, 80);
AT(pll_partition_t, rate_weights, 88);
AT(pll_partition_t, subst_params, 96);
AT(pll_partition_t, scale_buffer, 104);
AT(pll_partition_t, frequencies, 112);
AT(pll_partition_t, prop_invar, 120);
AT(pll_partition_t, invariant, 128);
AT(pll_partition_t, pattern_weights, 136);
AT(pll_partition_t, eigen_decomp_valid, 144);
AT(pll_partition_t, eigenvecs, 152);
AT(pll_partition_t, inv_eigenvecs, 160);
AT(pll_partition_t, eigenvals, 168);
AT(pll_partition_t, maxstates, 176);
AT(pll_partition_t, tipchars, 184);
AT(pll_partition_t, charmap, 192);
AT(pll_partition_t, ttlookup, 200);
AT(pll_partition_t, tipmap, 208);
AT(pll_partition_t, asc_bias_alloc, 216);
AT(pll_partition_t, asc_additional_sites, 220);
AT(pll_partition_t, repeats, 224);

_Static_assert(sizeof(pll_repeats_t) == 104, "pll_repeats_t size");
AT(pll_repeats_t, pernode_site_id, 0);
AT(pll_repeats_t, pernode_id_site, 8);
AT(pll_repeats_t, pernode_ids, 16);
AT(pll_repeats_t, perscale_ids, 24);
AT(pll_repeats_t, pernode_allocated_clvs, 32);
AT(pll_repeats_t, enable_repeats, 40);
AT(pll_repeats_t, reallocate_repeats, 48);
AT(pll_repeats_t, lookup_buffer, 56);
AT(pll_repeats_t, toclean_buffer, 64);
AT(pll_repeats_t, id_site_buffer, 72);
AT(pll_repeats_t, bclv_buffer, 80);
AT(pll_repeats_t, lookup_buffer_size, 88);
AT(pll_repeats_t, charmap, 96);

_Static_assert(sizeof(pll_operation_t) == 32, "pll_operation_t size");
AT(pll_operation_t, parent_clv_index, 0);
AT(pll_operation_t, parent_scaler_index, 4);
AT(pll_operation_t, child1_clv_index, 8);
AT(pll_operation_t, child1_matrix_index, 12);
AT(pll_operation_t, child1_scaler_index, 16);
AT(pll_operation_t, child2_clv_index, 20);
AT(pll_operation_t, child2_matrix_index, 24);
AT(pll_operation_t, child2_scaler_index, 28);
_Static_assert(sizeof(pll_state_t) == 8, "pll_state_t size");

/* src/pll.h:468-500 */
_Static_assert(sizeof(pll_parsimony_t) == 104, "pll_parsimony_t size");
AT(pll_parsimony_t, tips, 0);
AT(pll_parsimony_t, inner_nodes, 4);
AT(pll_parsimony_t, sites, 8);
AT(pll_parsimony_t, states, 12);
AT(pll_parsimony_t, attributes, 16);
AT(pll_parsimony_t, alignment, 24);
AT(pll_parsimony_t, packedvector, 32);
AT(pll_parsimony_t, node_cost, 40);
AT(pll_parsimony_t, packedvector_count, 48);
AT(pll_parsimony_t, const_cost, 52);
AT(pll_parsimony_t, informative, 56);
AT(pll_parsimony_t, informative_count, 64);
AT(pll_parsimony_t, score_buffers, 68);
AT(pll_parsimony_t, ancestral_buffers, 72);
AT(pll_parsimony_t, score_matrix, 80);
AT(pll_parsimony_t, sbuffer, 88);
AT(pll_parsimony_t, anc_states, 96);
_Static_assert(sizeof(pll_pars_buildop_t) == 12, "pll_pars_buildop_t size");
AT(pll_pars_buildop_t, parent_score_index, 0);
AT(pll_pars_buildop_t, child1_score_index, 4);
AT(pll_pars_buildop_t, child2_score_index, 8);
_Static_assert(sizeof(pll_pars_recop_t) == 16, "pll_pars_recop_t size");
AT(pll_pars_recop_t, node_score_index, 0);
AT(pll_pars_recop_t, node_ancestral_index, 4);
AT(pll_pars_recop_t, parent_score_index, 8);
AT(pll_pars_recop_t, parent_ancestral_index, 12);

/* this library's own: one candidate edge of pll_gpu_insertion_loglikelihoods */
_Static_assert(sizeof(pll_gpu_insertion_t) == 24, "pll_gpu_insertion_t size");
AT(pll_gpu_insertion_t, child1_clv_index, 0);
AT(pll_gpu_insertion_t, child1_scaler_index, 4);
AT(pll_gpu_insertion_t, child1_matrix_index, 8);
AT(pll_gpu_insertion_t, child2_clv_index, 12);
AT(pll_gpu_insertion_t, child2_scaler_index, 16);
AT(pll_gpu_insertion_t, child2_matrix_index, 20);
/* ... and one quartet of pll_gpu_quartet_loglikelihoods */
_Static_assert(sizeof(pll_gpu_quartet_t) == 52, "pll_gpu_quartet_t size");
AT(pll_gpu_quartet_t, clv_index, 0);
AT(pll_gpu_quartet_t, scaler_index, 16);
AT(pll_gpu_quartet_t, matrix_index, 32);
AT(pll_gpu_quartet_t, inner_matrix_index, 48);
/* ... and one branch of pll_gpu_branch_derivatives */
_Static_assert(sizeof(pll_gpu_branch_t) == 24, "pll_gpu_branch_t size");
AT(pll_gpu_branch_t, parent_clv_index, 0);
AT(pll_gpu_branch_t, parent_scaler_index, 4);
AT(pll_gpu_branch_t, child_clv_index, 8);
AT(pll_gpu_branch_t, child_scaler_index, 12);
AT(pll_gpu_branch_t, branch_length, 16);

/* the extension block must start 8-byte aligned directly behind the public struct */
_Static_assert(sizeof(pll_partition_t) % 8 == 0, "extension block alignment");

/* options and result of pll_gpu_optimize_branch_length, mirrored field for field by the device layer */
_Static_assert(sizeof(pll_gpu_newton_t) == 40 && sizeof(pllgpu_newton_t) == 40, "pll_gpu_newton_t size");
AT(pll_gpu_newton_t, tolerance, 24);
AT(pll_gpu_newton_t, max_iters, 32);
AT(pll_gpu_newton_t, matrix_index, 36);
_Static_assert(sizeof(pll_gpu_newton_result_t) == 40 && sizeof(pllgpu_newton_result_t) == 40, "pll_gpu_newton_result_t size");
AT(pll_gpu_newton_result_t, dd_f, 16);
AT(pll_gpu_newton_result_t, iterations, 24);
AT(pll_gpu_newton_result_t, host_waits, 28);
AT(pll_gpu_newton_result_t, status, 32);
_Static_assert(PLL_GPU_NEWTON_MAX_ITERS == PLLGPU_NEWTON_MAX_ITERS && PLL_GPU_NEWTON_MAXITER == PLLGPU_NEWTON_MAXITER, "Newton constants");

/* the outputs of pll_gpu_pairwise_distances, mirrored field for field by the device layer and by pllamd/api.py */
_Static_assert(sizeof(pll_gpu_distances_t) == 48 && sizeof(pllgpu_distances_t) == 48, "pll_gpu_distances_t size");
AT(pll_gpu_distances_t, distance, 0);
AT(pll_gpu_distances_t, p_distance, 8);
AT(pll_gpu_distances_t, d_f, 16);
AT(pll_gpu_distances_t, dd_f, 24);
AT(pll_gpu_distances_t, status, 32);
AT(pll_gpu_distances_t, iterations, 40);

/* the outputs of pll_gpu_bootstrap_distance_trees, likewise */
_Static_assert(sizeof(pll_gpu_bootstrap_trees_t) == 40 && sizeof(pllgpu_bootstrap_trees_t) == 40, "pll_gpu_bootstrap_trees_t size");
AT(pll_gpu_bootstrap_trees_t, parent, 0);
AT(pll_gpu_bootstrap_trees_t, length, 8);
AT(pll_gpu_bootstrap_trees_t, distances, 16);
AT(pll_gpu_bootstrap_trees_t, status, 24);
AT(pll_gpu_bootstrap_trees_t, weights, 32);

/* queries the Python binding declares by hand (pllamd/api.py): the prototypes it assumes */
_Static_assert(_Generic(&pll_gpu_pending_clvs, unsigned int (*)(const pll_partition_t *): 1, default: 0) &&
               _Generic(&pllgpu_pending_clvs, unsigned (*)(const pllgpu_ctx_t *): 1, default: 0), "pll_gpu_pending_clvs prototype");

/* the tree calls (nj.c): the public flag is the device layer's, and pllamd/api.py assumes these prototypes */
_Static_assert(PLL_GPU_NJ_BIONJ == PLLGPU_NJ_BIONJ, "NJ flags");
_Static_assert(_Generic(&pll_gpu_nj_tree, int (*)(const double *, unsigned int, unsigned int, int, int *, double *): 1, default: 0) &&
               _Generic(&pllgpu_nj_tree, int (*)(int, const double *, unsigned int, unsigned int, int *, double *): 1, default: 0),
               "pll_gpu_nj_tree prototype");
_Static_assert(_Generic(&pll_gpu_nj_last_launch_count, unsigned int (*)(void): 1, default: 0) &&
               _Generic(&pll_gpu_nj_last_device_ms, double (*)(void): 1, default: 0), "pll_gpu_nj_last_* prototypes");
