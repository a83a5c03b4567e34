/*
 * mkamd_distance.h -- C ABI of libmkamd.so, distance_utils row.
 *
 * GPU replacements for moleculekit/distance_utils/distance_utils.pyx:
 *   dist_trajectory                  :126-155     -> mkamd_dist_trajectory_host / _dev
 *   contacts_trajectory              :59-93  }    -> mkamd_contacts_trajectory_host / _dev (thresholded and compacted on the GPU,
 *   get_collisions                   :98-121 }       the reference's (frame, i, j) order; no [frames x pairs] matrix anywhere)
 *   dist_trajectory_reduction        :211-281 }   -> mkamd_dist_reduction_host / _dev (pairs = 0 / 1)
 *   dist_trajectory_reduction_pairs  :286-350 }
 *   cdist                            :355-383     -> mkamd_cdist_host / _dev
 *   pdist                            :388-416     -> mkamd_pdist_host / _dev
 * All float32, BIT-EXACT with the reference (same operation order, one rounding per operation).
 *
 * Layouts (C-contiguous, the reference's):  coords float32 [n_atoms, 3, n_frames] (Molecule.coords),
 * box float32 [3, n_frames] (Molecule.box), results float32 [n_frames, n_pairs].
 * Pair order: i over sel1, j over sel2 (from i+1 when selfdist) -- the reference's loop order.
 * n_frames < 2^30 (MKAMD_EINVAL beyond: a frame's byte offset into a coordinate row is a 32-bit buffer offset in the
 * kernels; the reference's own frame loops are C ints).
 * Host pointers in, host pointers out (copies + kernels + synchronise); status codes as mkamd_voxel.h.
 */
#ifndef MKAMD_DISTANCE_H
#define MKAMD_DISTANCE_H

#include "mkamd_voxel.h"

#ifdef __cplusplus
extern "C" {
#endif

/* number of (i,j) pairs the reference's loops visit (n1*n2, or sum_i max(n2-1-i,0) when selfdist) */
int64_t mkamd_dist_count_pairs(int64_t n1, int64_t n2, int selfdist);

/* dist_trajectory(coords, box, sel1, sel2, digitized_chains, selfdist, pbc, results);  squared != 0
 * stores the squared distance (what contacts_trajectory compares with threshold^2) instead of its sqrt. */
int mkamd_dist_trajectory_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames,
                               const float* box, const uint32_t* sel1, int64_t n1, const uint32_t* sel2,
                               int64_t n2, const uint32_t* digitized_chains, int selfdist, int pbc,
                               int squared, float* results);
/* same on device pointers (asynchronous on the context's stream) */
int mkamd_dist_trajectory_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_frames, const float* d_box,
                              const uint32_t* d_sel1, int64_t n1, const uint32_t* d_sel2, int64_t n2,
                              const uint32_t* d_digitized_chains, int selfdist, int pbc, int squared,
                              float* d_results);

/* contacts_trajectory(coords, box, sel1, sel2, digitized_chains, selfdist, pbc, dist_threshold): per frame the atom
 * pairs (a, b) = (sel1[i], sel2[j]) with dist2 <= threshold^2 (float32 compare, distance_utils.pyx:73,82), in the
 * reference's (i, j) loop order.  Counted, prefix-summed and written on the device, chunk of frames by chunk of frames
 * (memory stays bounded whatever n_frames x n_pairs is).
 *   frame_offsets int64 [n_frames + 1] (out): frame f owns pairs [frame_offsets[f], frame_offsets[f+1])
 *   *pairs (out): 2 * frame_offsets[n_frames] uint32 (a0, b0, a1, b1, ...) in memory OWNED BY THE CONTEXT, valid until
 *   the next contacts call on it (NULL when there is no contact).
 * get_collisions (:98-121) is the one-frame, non-periodic case on the concatenation of the two coordinate sets. */
int mkamd_contacts_trajectory_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames,
                                   const float* box, const uint32_t* sel1, int64_t n1, const uint32_t* sel2,
                                   int64_t n2, const uint32_t* digitized_chains, int selfdist, int pbc,
                                   float dist_threshold, int64_t* frame_offsets, const uint32_t** pairs);

/* dist_trajectory_reduction / dist_trajectory_reduction_pairs.  The reference's vector<vector<int>> groups
 * are passed as CSR: atoms int32 [sum of group sizes], offsets int64 [n_groups + 1].  reduction: 0 closest,
 * 1 centre of mass (masses float32 [n_atoms]).  results float32 [n_frames, n_out], n_out = n_groups1 when
 * pairs else mkamd_dist_count_pairs(n_groups1, n_groups2, selfdist). */
int mkamd_dist_reduction_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames,
                              const float* box, const int32_t* g1_atoms, const int64_t* g1_offsets,
                              int64_t n_groups1, const int32_t* g2_atoms, const int64_t* g2_offsets,
                              int64_t n_groups2, const uint32_t* digitized_chains1,
                              const uint32_t* digitized_chains2, int selfdist, int pairs, int pbc,
                              const float* masses, int reduction1, int reduction2, float* results);

/* ---- device-resident forms (round 6): device pointers in, device results out, on the context's stream (mkamd_ctx_set_stream)
 * -- for callers that keep the trajectory on the GPU (a decoded XTC chunk, an ML / analysis loop).  Same kernels, same bits as the
 * "_host" forms.  Asynchronous like mkamd_dist_trajectory_dev, except the contact list (its size has to reach the host). ---- */

/* contacts_trajectory (distance_utils.pyx:59-93) on device pointers: frame_offsets is a HOST array int64 [n_frames + 1] (out);
 * *d_pairs (out) points at 2 * frame_offsets[n_frames] uint32 (a0, b0, a1, b1, ...) in DEVICE memory owned by the context, valid
 * until the next contacts call on it (NULL when there is no contact).  The call returns when the list is complete. */
int mkamd_contacts_trajectory_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_frames, const float* d_box,
                                  const uint32_t* d_sel1, int64_t n1, const uint32_t* d_sel2, int64_t n2,
                                  const uint32_t* d_digitized_chains, int selfdist, int pbc, float dist_threshold,
                                  int64_t* frame_offsets, const uint32_t** d_pairs);
/* dist_trajectory_reduction[_pairs] (:211-350) on device pointers.  n_atoms (rows of d_coords) and n_g1_atoms (length of
 * d_g1_atoms = the value of d_g1_offsets[n_groups1]) are what the host knows about the device arrays: they choose the kernel
 * variant (32-bit row offsets, first-group atoms per wave), never the result.  Indices are NOT range-checked on the device. */
int mkamd_dist_reduction_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t n_frames, const float* d_box,
                             const int32_t* d_g1_atoms, const int64_t* d_g1_offsets, int64_t n_groups1, int64_t n_g1_atoms,
                             const int32_t* d_g2_atoms, const int64_t* d_g2_offsets, int64_t n_groups2,
                             const uint32_t* d_digitized_chains1, const uint32_t* d_digitized_chains2, int selfdist, int pairs,
                             int pbc, const float* d_masses, int reduction1, int reduction2, float* d_results);
/* cdist (:355-383) / pdist (:388-416) on device pointers */
int mkamd_cdist_dev(mkamd_ctx* ctx, const float* d_coords1, int64_t n1, const float* d_coords2, int64_t n2, int32_t dim,
                    float* d_results);
int mkamd_pdist_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n, int32_t dim, float* d_results);

/* Self-test of the kernels' float32 square root.  The reference's sqrtf is correctly rounded; the kernels take roots with
 * one exact-residual correction of x * rsq(x) (8 issue slots; the provable form, v_sqrt_f32 + Tuckerman's test, takes 12 and
 * the kernels are bound by instruction issue).  That this is the correctly rounded root is a property of gfx950's v_rsq_f32,
 * checked rather than proved: this call compares the two forms on the device over EVERY float in [2^-96, inf) -- 1.9e9 values,
 * a few milliseconds -- and returns the number of mismatches (0 on the hardware this library is built for) and the bit pattern
 * of the first one.  Run by the GPU test tier. */
int mkamd_selftest_sqrt(mkamd_ctx* ctx, uint64_t* mismatches, uint32_t* first_bad_bits);

/* Self-test of the device arithmetic under the bit-exact kernels (csrc/arith_probe.h): operation `op` applied elementwise to n
 * elements of the device arrays a, b, c (those the operation reads; the others may be NULL) into the device array `out`, by a
 * kernel that calls the very function the product's kernels call.  The element width is fixed by the operation:
 *    0 fadd, 1 fsub, 2 fmul (a, b), 3 fmul_add (a * b + c, two roundings), 5 fdiv, 6 ring_div, 13 round(a / b) of the distance
 *    kernels, 19 the rings' round(a / b), 14 the squared minimum-image separation of a in a box b, 16 the dihedrals' wrap of a
 *    in a box b, 8 fsqrt, 9 ring_sqrt, 10 roundf, 11 rint, 17 the restated acosf: float32 in, float32 out;
 *    20 the same separation and its negative through the packed form (dist2_pk): float32 in, THREE float32 out per element (the two
 *    squared separations; 1 where the accumulated test tells the caller to redo the pair with the form of 14, else 0);
 *    15 the wrap's decision (group centre a, box centre b, box c): float32 in, TWO float32 out per element (1 or 0: moved; the translation);
 *    12 round((double)a), 18 the folded angle in degrees of a: float32 in, float64 out;
 *    4 dmul_add (a * b + c, two roundings), 7 ddiv: float64 in, float64 out.
 * Consecutive elements are consecutive lanes (64 to a wave, 256 to a block).  Launched on the context's stream; the call does not
 * wait.  Run by the GPU test tier against independent references, bit for bit. */
int mkamd_selftest_arith(mkamd_ctx* ctx, int op, long long n, const void* a, const void* b, const void* c, void* out);

/* Which kernels dist_trajectory may take (default 0: all; the choice depends on the shape of the call): bits of `avoid_mask` --
 * 1 the block-per-frame kernel (rectangular calls with short rows -- the small calls MetricDistance makes: one launch), 2 the row
 * kernel (rectangular calls with rows of >= 64 second atoms), 4 the rectangular tile kernel, 8 the row kernel's 16-byte stores,
 * 16 (not an exclusion) the row kernel wherever it applies, also where the tile kernel is the measured better choice
 * (selfdist always takes the pair-table kernel); 32 (not a kernel): the host entry points upload the whole coordinate array instead
 * of the selected atoms' rows (csrc/host_pack.h); 64: selfdist calls keep the pair-table kernel where the triangular form of the row kernel
 * would be taken (selections of >= 700 atoms up to 32 frames, of >= 1 500 atoms at any frame count).  128: rectangular calls of few frames whose rows are too short for the row kernel and whose first selection is long keep the tile
 * kernel instead of the row kernel with the selections swapped (lanes along the first selection, transposed stores).
 * 256 / 512: shell counts do not take their frame-lane / atom-lane kernel; 1024 / 2048: the dihedral angles the same.
 * 4096 / 8192: the group moments do not take the form in which a lane group owns a whole (frame, group) / the segmented form.
 * 16384 / 32768: the periodic wrap does not take the lane-per-group kernel (every group a wave) / the wave-per-group kernel (every
 * group a lane).
 * Calls of at most 32 frames take the row kernel wherever it applies (its lanes
 * run along the second atoms; the other kernels' along frames).  Every kernel produces the same
 * bits; for tests (every kernel over the same shapes) and same-box A-B timing. */
int mkamd_ctx_set_dist_kernels(mkamd_ctx* ctx, int avoid_mask);
/* Which kernel the "closest"/"closest" group reductions take (default 0: k_dist_reduction_closest with 4 or 8 first-group atoms in
 * registers, chosen from the mean size of the first groups -- and, for calls of at most 16 frames (8 when not periodic) in any reduction mode,
 * k_dist_reduction_few, whose lanes run along the second groups instead of the frames; 4 / 8: that many (+ 100: in blocks of four
 * waves instead of eight); -1: the generic kernel the centre-of-mass modes use; -2: the few-frame kernel at any number of frames).
 * Every choice produces the same bits; for tests and same-box A-B timing. */
int mkamd_ctx_set_reduction_block(mkamd_ctx* ctx, int block);
/* Names of the kernels the last dist_trajectory call on this context launched, as a profiler prints them (e.g.
 * "mkamd::k_sel_to_frames + mkamd::k_dist_rows<true, 4, true>"; empty before the first call): what bench.py reports as
 * the distance leg's `roofline.kernel` -- the choice depends on the shape of the call.  The shell, dihedral, moment and alignment
 * calls note theirs the same way (alignment: "mkamd::k_align_sums<AL_MATCH> G=64 segs=16 + mkamd::k_align_fold<17, 24>" -- the
 * sums' mode, the lanes per frame, and the fold exactly when the frames' selection was cut into segments), and so do the
 * explicit-centre occupancy calls of mkamd_voxel.h ("mkamd::k_occupancy_centers, 8 waves": the workgroup width -- 4, 8 or 16 waves --
 * that the number of centres and channels chose). */
int mkamd_ctx_last_dist_kernel(mkamd_ctx* ctx, char* name, size_t name_cap);

/* cdist(coords1 [n1,D], coords2 [n2,D]) -> results [n1,n2];  pdist(coords [n,D]) -> results [n(n-1)/2] */
int mkamd_cdist_host(mkamd_ctx* ctx, const float* coords1, int64_t n1, const float* coords2, int64_t n2,
                     int32_t dim, float* results);
int mkamd_pdist_host(mkamd_ctx* ctx, const float* coords, int64_t n, int32_t dim, float* results);

/* ---- alignment: rigid superposition of frames on a reference structure (moleculekit align.py _pp_align / Molecule.align,
 * the RMSD of projections/metricrmsd.py) ----
 * Device layout: frame-major float32 d_xyz [n_frames, n_atoms, 3] (the XTC decoder's and the voxelizer's items), the reference
 * d_ref [n_ref_frames, n_ref_atoms, 3].  d_sel / d_refsel uint32 [n_sel]: the alignment pairs atom d_sel[k] of a frame with atom
 * d_refsel[k] of the reference (indices NOT range-checked on the device).  d_frames int64 [n_list] (NULL: frames 0 .. n_list - 1)
 * lists the frames; entry i of every per-frame output belongs to d_frames[i].  The reference frame is `refframe`, or with
 * `matchingframes` the listed frame's own index (then n_ref_frames == n_frames).
 * Transform i is the optimal PROPER rotation in the least-squares sense (Horn's quaternion; no reflection) as affine float64
 * [12] = row-major R, then t = c_Q - R c_P -- the layout of mkamd_voxelize_lattice_aug_dev's d_affine (mkamd_voxel.h (3b)), so
 * it can be handed to the voxelizer as is.  Everything is summed in double in a fixed order: the same bits on every run.
 * An empty selection gives R = I and NaN translations (the reference's means of nothing), not an error.  Asynchronous on the
 * context's stream. */

/* d_affine [n_list, 12] (out), d_fit_rmsd [n_list] (out, nullable): sqrt(max(0, E_P + E_Q - 2 lambda_max) / n_sel) */
int mkamd_align_transforms_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t n_atoms, int64_t n_frames, const float* d_ref,
                               int64_t n_ref_atoms, int64_t n_ref_frames, const uint32_t* d_sel, const uint32_t* d_refsel,
                               int64_t n_sel, const int64_t* d_frames, int64_t n_list, int64_t refframe, int matchingframes,
                               double* d_affine, double* d_fit_rmsd);
/* d_out[f] = float32(R x + t) (evaluated in double, the voxelizer's operation order) for every atom x of each listed frame
 * f = d_frames[i] with transform d_affine[i]; other frames of d_out are not touched.  d_out may be d_xyz (in place). */
int mkamd_align_apply_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t n_atoms, const int64_t* d_frames, int64_t n_list,
                          const double* d_affine, float* d_out);
/* d_rmsd [n_list] float32 (out): sqrt(sum_k |float32(R p_k + t) - q_k|^2 / n_sel) over the pairs (d_sel, d_refsel), summed in
 * double and rounded once -- util.molRMSD of the aligned frame, without writing the aligned coordinates anywhere. */
int mkamd_align_rmsd_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t n_atoms, int64_t n_frames, const float* d_ref,
                         int64_t n_ref_atoms, int64_t n_ref_frames, const uint32_t* d_sel, const uint32_t* d_refsel, int64_t n_sel,
                         const int64_t* d_frames, int64_t n_list, int64_t refframe, int matchingframes, const double* d_affine,
                         float* d_rmsd);
/* align.py _pp_align(coords, refcoords, sel, refsel, frames, refframe, matchingframes, inplace=True) on host arrays in the
 * reference's layout: coords float32 [n_atoms, 3, n_frames] (Molecule.coords), refcoords [n_ref_atoms, 3, n_ref_frames].  Only the
 * span of frames between the smallest and the largest listed one is uploaded (and the reference's frame, or its listed frames);
 * only the listed frames of coords are written.  Every input is read before anything is written, so refcoords may be coords. */
int mkamd_align_host(mkamd_ctx* ctx, float* coords, int64_t n_atoms, int64_t n_frames, const float* refcoords, int64_t n_ref_atoms,
                     int64_t n_ref_frames, const uint32_t* sel, const uint32_t* refsel, int64_t n_sel, const int64_t* frames,
                     int64_t n_list, int64_t refframe, int matchingframes);

/* ---- surface area: the solvent-accessible surface of every frame (Shrake-Rupley; moleculekit projections/metricsasa.py, which
 * calls mdtraj's sasa.cpp) ----
 * Per frame and per atom i whose mask is non-zero: R_i = radii[i] (probe included); the neighbours of i are all j != i with
 * |x_i - x_j|^2 < (R_i + R_j)^2; of the n_points sphere points p = x_i + R_i s (the reference's golden-section spiral) the ones
 * with |p - x_j|^2 < R_j^2 for no neighbour j are counted, and area_i = ((float32(4 pi / n_points) * count) * R_i) * R_i is added
 * to out[frame, atom_mapping[i]].  Every atom shields, selected or not.  All of it in float32 with separate multiplies and adds
 * (|d|^2 = (dx dx + dy dy) + dz dz): the count is the reference's exactly.  Coordinates are divided by `coord_div` first (IEEE
 * division; 10: Angstrom in, the reference's nanometres inside -- radii are then nanometres and the areas square nanometres;
 * 1: as they are).  atom_mapping int32: inside [0, n_out) and NON-DECREASING (the atoms of a column are contiguous; a column's
 * areas are added one after the other in atom order, no floating-point atomics: the same bits on every run); mask int32.
 * out [n_frames, n_out] float32 is filled by the caller; columns no selected atom maps to are left alone.
 * Refused with MKAMD_EINVAL, nothing added to out: two atoms with r^2 < 1e-10 in the divided coordinates (the reference aborts
 * the process there), a mapping value out of range or smaller than its predecessor.  Both calls return after the kernels have
 * finished (the refusal flag is read back). */

/* device arrays: d_xyz frame-major [n_frames, n_atoms, 3] (the XTC decoder's and the voxelizer's items), on the context's stream */
int mkamd_sasa_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t n_atoms, int64_t n_frames, const float* d_radii, int32_t n_points,
                   const int32_t* d_atom_mapping, const int32_t* d_mask, float coord_div, float* d_out, int64_t n_out);
/* host arrays: coords [n_atoms, 3, n_frames] (Molecule.coords); keep uint32 [n_keep] lists the atoms of the system (NULL: all
 * n_atoms) -- only their rows are uploaded; radii, atom_mapping and mask are [n_keep], in the order of keep. */
int mkamd_sasa_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const uint32_t* keep, int64_t n_keep,
                    const float* radii, int32_t n_points, const int32_t* atom_mapping, const int32_t* mask, float coord_div,
                    float* out, int64_t n_out);

/* ---- shell counts: how many atoms of sel2 lie in each of n_edges - 1 concentric shells around every atom of sel1, per frame
 * (moleculekit projections/metricshell.py) -- without the [n_frames, n1 * n2] distance matrix the reference histograms ----
 * Layouts of the distance row: coords [n_atoms, 3, n_frames], box [3, n_frames], sel1 / sel2 / digitized_chains uint32.  For frame
 * f, centre i and atom j: d2 = the squared float32 minimum-image distance of dist_trajectory (the image shift where pbc is set and
 * digitized_chains[sel1[i]] != digitized_chains[sel2[j]]), and counts[f, i, s] = #{ j : T[s] < d2 <= T[s + 1] } with the
 * non-decreasing float32 thresholds T = d2_thresholds [n_edges] (+inf allowed; a NaN d2 is in no shell).  The thresholds are on the
 * SQUARED distance: for a shell edge e, T is the largest float32 whose correctly rounded root is <= e, and then d2 <= T is exactly
 * fl32(sqrt(d2)) <= e (the rounded root is monotone) -- moleculekit_amd.shell.shell_thresholds computes them.  symmetric: sel1 and
 * sel2 are the same list (n1 == n2) and the pair (i, i) is left out.  counts int32 [n_frames, n1, n_edges - 1] is cleared by the
 * call; integer sums: the same on every run.  n_edges 2 .. 33 (1 .. 32 shells), n_frames < 2^30; else MKAMD_EINVAL.  No workspace
 * proportional to n1 * n2 exists anywhere. */

/* device arrays, asynchronous on the context's stream; d2_thresholds is HOST memory, read before the call returns */
int mkamd_shell_counts_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t n_frames, const float* d_box,
                           const uint32_t* d_sel1, int64_t n1, const uint32_t* d_sel2, int64_t n2, const uint32_t* d_digitized_chains,
                           int symmetric, int pbc, const float* d2_thresholds, int64_t n_edges, int32_t* d_counts);
/* host arrays: only the selected atoms' rows are uploaded (as the other host forms do); returns when counts is filled */
int mkamd_shell_counts_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const float* box,
                            const uint32_t* sel1, int64_t n1, const uint32_t* sel2, int64_t n2, const uint32_t* digitized_chains,
                            int symmetric, int pbc, const float* d2_thresholds, int64_t n_edges, int32_t* counts);

/* ---- dihedral angles: the torsion of n_dihedrals atom quadruples in every frame (moleculekit projections/metricdihedral.py:
 * _calcDihedralAngles -> dihedral.py:dihedralAngle) ----
 * coords [n_atoms, 3, n_frames] float32, quads uint32 [n_dihedrals, 4] (indices < n_atoms), box [3, n_frames] float32 or NULL (then
 * n_box_frames is not read; else it must equal n_frames).  For atoms x0..x3: r12 = x0 - x1, r23 = x1 - x2, r34 = x2 - x3 -- with a
 * box each component once through the reference's _wrapBondedDistance (< -box / 2: + box; > box / 2: - box; a box of zeros changes
 * nothing) --, c1 = r23 x r34, c2 = r12 x r23, p1 = (r12 . c1) * sqrt(r23 . r23), p2 = c1 . c2: the reference's float32 operations
 * in its order, no fused multiply-add, the root correctly rounded -- (p1, p2) are its bits.  The angle is -atan2(p1, p2).  `mode`:
 *   MKAMD_DIH_TERMS 0    out [n_frames, n_dihedrals, 2]   (p1, p2)
 *   MKAMD_DIH_RADIANS 1  out [n_frames, n_dihedrals]      the float64 atan2 of the terms, rounded once to float32
 *   MKAMD_DIH_DEGREES 2  out [n_frames, n_dihedrals]      the same times 180 / pi in float64, rounded once
 *   MKAMD_DIH_SINCOS 3   out [n_frames, 2 n_dihedrals]    sin, cos interleaved: (-p1, p2) / sqrt(p1^2 + p2^2) in float64, rounded once
 * p1 = p2 = 0 (collinear atoms): angle 0, sin 0, cos 1.  A NaN coordinate gives NaN in every output of that (frame, dihedral) only.
 * MKAMD_EINVAL: an unknown mode, a NULL pointer, n_box_frames != n_frames, n_frames or n_dihedrals >= 2^30, (host form) an index
 * >= n_atoms.  No workspace proportional to n_frames * n_dihedrals besides the result. */
enum { MKAMD_DIH_TERMS = 0, MKAMD_DIH_RADIANS = 1, MKAMD_DIH_DEGREES = 2, MKAMD_DIH_SINCOS = 3 };

/* device arrays, asynchronous on the context's stream; the indices are NOT checked (they are device memory) */
int mkamd_dihedrals_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t n_frames, const float* d_box, int64_t n_box_frames,
                        const uint32_t* d_quads, int64_t n_dihedrals, int mode, float* d_out);
/* host arrays: only the rows of the atoms the quads name are uploaded (as the other host forms do); returns when out is filled */
int mkamd_dihedrals_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const float* box, int64_t n_box_frames,
                         const uint32_t* quads, int64_t n_dihedrals, int mode, float* out);

/* ---- group moments: weighted first and second moments of small sets of atoms in every frame, optionally after each frame's rigid
 * transform (moleculekit projections/metriccoordinate.py, metricgyration.py, metricsphericalcoordinate.py, metricfluctuation.py) ----
 * Device layout: frame-major float32 d_xyz [n_frames, n_atoms, 3] (the alignment's).  d_affine float64 [n_frames, 12] or NULL: what
 * mkamd_align_transforms_dev writes for frames 0 .. n_frames - 1; every gathered atom is then float32(R x + t) first -- the bits
 * mkamd_align_apply_dev would have stored, and the aligned trajectory is never written.  Groups are CSR: atoms uint32 [n_sel]
 * (indices < n_atoms), offsets uint32 [n_groups + 1] (offsets[0] = 0, offsets[n_groups] = n_sel, no empty group), weights float32
 * [n_sel] or NULL (1).  max_group: the largest group's size (it shapes the launch only).  Per (frame, group) everything is summed in
 * double, in a fixed order, without floating-point atomics: the same bits on every run.  `mode`:
 *   MKAMD_MOM_CENTER 0     out float32 [n_frames, 3 n_groups], column c * n_groups + g:  sum w x_c / sum w, rounded once
 *   MKAMD_MOM_GYRATION 1   out float32 [n_frames, n_groups, 4]: sqrt(sum w q / sum w) for q = |r|^2, r_y^2 + r_z^2, r_x^2 + r_z^2,
 *                          r_x^2 + r_y^2 with r = x - (centre of mass), the centre kept in double; rounded once
 *   MKAMD_MOM_SPHERICAL 2  exactly two unweighted groups (target, reference): d = centroid_0 - centroid_1 in double,
 *                          out float32 [n_frames, 3] = (|d|, acos(d_z / |d|), atan2(d_y, d_x)); |d| = 0 gives NaN for the second
 *   MKAMD_MOM_FLUCT 3      (mkamd_fluctuation_*) out FLOAT64 [n_frames, n_sel] = sum_c (x_c - ref_c)^2 per listed atom, or with
 *                          offsets [n_frames, n_groups]: its unweighted mean over each group's atoms.  ref float64 [n_sel, 3], or NULL:
 *                          the mean over all frames of the (transformed) positions, computed first in double in a fixed order
 * MKAMD_EINVAL: an unknown mode, a NULL pointer, n_frames, n_groups or n_sel >= 2^30, the spherical mode with other than two groups or with
 * weights, (host forms) an index >= n_atoms, an empty group, offsets that do not start at 0 or decrease. */
enum { MKAMD_MOM_CENTER = 0, MKAMD_MOM_GYRATION = 1, MKAMD_MOM_SPHERICAL = 2, MKAMD_MOM_FLUCT = 3 };

/* device arrays, asynchronous on the context's stream; indices and offsets are NOT checked (they are device memory) */
int mkamd_group_moments_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t n_atoms, int64_t n_frames, const double* d_affine,
                            const uint32_t* d_atoms, const uint32_t* d_offsets, const float* d_weights, int64_t n_groups, int64_t n_sel,
                            int64_t max_group, int mode, float* d_out);
/* d_offsets NULL: per atom (n_groups and max_group are not read); d_ref NULL: the mean over the frames */
int mkamd_fluctuation_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t n_atoms, int64_t n_frames, const double* d_affine,
                          const uint32_t* d_atoms, int64_t n_sel, const uint32_t* d_offsets, int64_t n_groups, int64_t max_group,
                          const double* d_ref, double* d_out);
/* host arrays: coords float32 [n_atoms, 3, n_frames] (Molecule.coords).  alnsel uint32 [n_aln] with alnref float32 [n_aln, 3], or
 * NULL: every frame is first superposed (mkamd_align_transforms_dev) with its atoms alnsel on the positions alnref.  Only the rows of
 * the atoms that atoms and alnsel name are packed and uploaded; returns when out is filled. */
int mkamd_group_moments_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const uint32_t* alnsel,
                             const float* alnref, int64_t n_aln, const uint32_t* atoms, const uint32_t* offsets, const float* weights,
                             int64_t n_groups, int mode, float* out);
/* ref float64 [n_sel, 3] or NULL (the mean over the frames); offsets NULL: per atom */
int mkamd_fluctuation_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const uint32_t* alnsel,
                           const float* alnref, int64_t n_aln, const uint32_t* atoms, int64_t n_sel, const uint32_t* offsets,
                           int64_t n_groups, const double* ref, double* out);

/* ---- periodic wrap: every bonded group of every frame back into the rectangular cell around a centre (moleculekit
 * wrapping/wrapping.pyx wrap_box, called from Molecule.wrap with boxangles of 90) ----
 * Device layout: frame-major float32 d_xyz [n_frames, n_atoms, 3], d_box float32 [3, n_frames].  Groups are contiguous runs of atoms:
 * d_starts uint32 [n_groups + 1], starts[0] = 0, increasing, starts[n_groups] = n_atoms.  Per frame the box centre is the float32
 * running mean c = c + (x - c) / float(n + 1) over the atoms d_centersel uint32 [n_centersel] of the UNWRAPPED frame, in the order
 * given -- or, with n_centersel == 0, the three floats `center` (host memory, read before the call returns).  Per group the same
 * running mean over its atoms in order; per axis i, diff = group centre - box centre: where fabs(diff) > box_i / 2, every atom of
 * the group gets x_i - float(double(box_i) * round(double(diff / box_i))) (float32 quotient, IEEE division, C's round).  Each
 * operation is rounded on its own: the results are the reference's bits.  A zero box length, a NaN or an infinite coordinate give
 * what that arithmetic gives.  d_out may be d_xyz (in place: groups that do not move are not written; the centres are complete
 * before any group is written) or a separate array of the same shape (every atom is written).
 * d_large uint32 [n_large]: the groups of more than mkamd_wrap_small_max(ctx) atoms, which a wave each handles instead of a lane
 * (a group listed that is not one is skipped; one that is missing is not wrapped).
 * MKAMD_EINVAL: a NULL pointer, a negative size, n_atoms or n_frames >= 2^30, more groups than atoms; (host form) starts that do not
 * begin at 0, do not increase or do not end at the number of atoms, an index >= n_atoms, rows that do not increase, a centre atom
 * that is not among the rows.  The device form does not check indices (they are device memory) but never reads or writes past
 * n_atoms: group bounds are clamped, a centre index >= n_atoms reads as NaN. */
int64_t mkamd_wrap_small_max(mkamd_ctx* ctx);
/* asynchronous on the context's stream */
int mkamd_wrap_box_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t n_atoms, int64_t n_frames, const float* d_box, const uint32_t* d_starts,
                       int64_t n_groups, const uint32_t* d_large, int64_t n_large, const uint32_t* d_centersel, int64_t n_centersel,
                       const float* center, float* d_out);
/* host arrays: coords float32 [n_atoms, 3, n_frames] (Molecule.coords), box [3, n_frames].  rows NULL: every atom travels, starts
 * [n_groups + 1] end at n_atoms and out is [n_atoms, 3, n_frames] (it may be coords).  rows uint32 [n_rows], strictly increasing: only
 * these atoms' rows are packed and uploaded (csrc/host_pack.h); starts then cut the ROWS into groups (they end at n_rows) and out is
 * [n_rows, 3, n_frames].  centersel names atoms of coords in either case (each must be among the rows).  Returns when out is filled. */
int mkamd_wrap_box_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const float* box, const uint32_t* rows,
                        int64_t n_rows, const uint32_t* starts, int64_t n_groups, const uint32_t* centersel, int64_t n_centersel,
                        const float* center, float* out);

/* ---- periodic wrap of TRICLINIC boxes: the three unit cells of Molecule.wrap when a box angle is not 90 (moleculekit
 * wrapping/wrapping.pyx wrap_compact_unitcell with mode 0 "rectangular" and mode 1 "compact", wrap_triclinic_unitcell: mode 2) ----
 * Everything as for mkamd_wrap_box_dev / _host but the box: d_boxvectors float64 [3, 3, n_frames], row i the box vector i, lower
 * triangular (box[0][1] = box[0][2] = box[1][2] = 0).  Every atom of a frame is first recentred, xc = (x - centre) + box_middle in
 * float32 (box_middle[j] = float(double(box_middle[j]) + 0.5 box[i][j])); group centres are the float32 running means over xc.
 * mode 2: the group's centre is moved by whole box vectors, for m = 2, 1, 0, until its fractional coordinate m lies in [0, 1) (GROMACS'
 * put_atoms_in_triclinic_unitcell: float64 shifts, the float32 centre rounded after every step); atoms get x_m = xc_m - (centre before -
 * centre after).  mode 0, 1: dx = double(group centre - box_middle) is brought into (-box[i][i] / 2, box[i][i] / 2] per axis by the
 * diagonal (mode 0) or by whole box vectors followed by the search over the frame's up to 12 triclinic vectors (mode 1: GROMACS'
 * pbc_dx); atoms get float(double((xc - group centre) + box_middle) + dx).  Each operation is rounded on its own: the results are the
 * reference's bits.  Every atom is written, in place (d_out == d_xyz) as out of place.
 * Where the reference's loops would not end, these do: each stops after mkamd_wrap_cell_max_steps() steps (one box vector a step)
 * and the group is written with what was reached; a frame with a non-finite box vector, box[1][1] or box[2][2] not positive or a
 * non-zero upper triangle is copied through unchanged.  d_status int [3] (or NULL) is cleared by the call and then holds 1 in
 * [0] where a loop reached that cap, [1] where a frame was copied through, [2] where a frame has more than 12 triclinic vectors (it is
 * copied through as well; the reference raises "Too many triclinic vectors!!").  The host form refuses such box vectors before it
 * launches anything and returns MKAMD_EINVAL, with a message that names the condition, where a status word is set (out is filled).
 * MKAMD_EINVAL besides: a mode other than 0, 1, 2, and everything mkamd_wrap_box_dev / _host refuse. */
int64_t mkamd_wrap_cell_max_steps(void);
/* asynchronous on the context's stream */
int mkamd_wrap_cell_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t n_atoms, int64_t n_frames, const double* d_boxvectors,
                        const uint32_t* d_starts, int64_t n_groups, const uint32_t* d_large, int64_t n_large, const uint32_t* d_centersel,
                        int64_t n_centersel, const float* center, int mode, float* d_out, int* d_status);
/* host arrays as for mkamd_wrap_box_host; boxvectors float64 [3, 3, n_frames].  Returns when out is filled. */
int mkamd_wrap_cell_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const double* boxvectors,
                         const uint32_t* rows, int64_t n_rows, const uint32_t* starts, int64_t n_groups, const uint32_t* centersel,
                         int64_t n_centersel, const float* center, int mode, float* out);

/* ---- ring interactions: pi-pi stacking, cation-pi and sigma-hole contacts of every frame (moleculekit interactions/pipi/pipi.pyx,
 * cationpi/cationpi.pyx, sigmahole/sigmahole.pyx: `calculate`) ----
 * kind 0 pi-pi: every ring of list 1 against every ring of list 2; 1 cation-pi: every ring against every cation; 2 sigma-hole: every
 * ring against every (halogen, bonded atom) pair.  The arguments are `calculate`'s:
 *   ring_atoms uint32 [n_ring_atoms]   the rings' atoms, concatenated (pi-pi: both lists, as the reference's wrapper builds them)
 *   starts1 uint32 [n1 + 1]            offsets of the rings of list 1 into ring_atoms; every ring has at least 3 atoms
 *   starts2 uint32 [n2 + 1]            kind 0: the same for list 2 (NULL otherwise).  A pair of rings with the same (start, end) is
 *                                      skipped, as in the reference -- whose wrapper shifts list 2 behind list 1, so that a ring named in
 *                                      both lists DOES pair with itself
 *   partners uint32 [n2] / [n2, 2]     kind 1: the cations; kind 2: (halogen, bonded atom) rows (NULL for kind 0)
 *   thresholds float [4], host         kind 0: dist_threshold1, angle_threshold1_max, dist_threshold2, angle_threshold2_min; kinds 1, 2:
 *                                      dist_threshold, angle_threshold_min (the other two are not read).  Distances are squared in float32
 * box float32 [3, n_frames]: the minimum image is applied per axis only where |d| > box / 2 and box != 0 (a zero axis is open; there is
 * no pbc flag); box NULL: every axis open.  Every float32 operation up to the squared distance and the dot product is the reference's,
 * rounded on its own; the angle is acos in float64 times 57.29578, folded at 90 (kinds 1, 2: 90 minus it).  A NaN angle fails every
 * comparison: the pair is dropped, as the reference drops it.
 * Results, the reference's order (frame; ring of list 1; partner): frame_offsets int64 [n_frames + 1] (host); *pairs uint32 [2 n]: the
 * ring's index in list 1 and the ring's index in list 2 (kind 0) / the cation's or halogen's ATOM index; *distang float32 [2 n]:
 * distance and angle in degrees.  Both lists are context-owned (NULL when n = 0) and valid until the next ring call on the context.
 * _dev: device pointers (coords [n_atoms, 3, n_frames]); the atom indices are NOT checked; the lists are device memory.  Not
 * asynchronous: the counts reach the host to size the lists.  MKAMD_EINVAL: a kind other than 0, 1, 2; a ring of fewer than 3 atoms;
 * offsets that decrease or leave ring_atoms; a NaN threshold; more than 2^30 pairs or frames. */
int mkamd_ring_interactions_dev(mkamd_ctx* ctx, int kind, const float* d_coords, int64_t n_atoms, int64_t n_frames, const float* d_box,
                                const uint32_t* d_ring_atoms, int64_t n_ring_atoms, const uint32_t* d_starts1, int64_t n1,
                                const uint32_t* d_starts2, const uint32_t* d_partners, int64_t n2, const float* thresholds,
                                int64_t* frame_offsets, const uint32_t** d_pairs, const float** d_distang);
/* host arrays; every atom index is checked against n_atoms (MKAMD_EINVAL); only the rows of the rings' and partners' atoms are packed
 * and uploaded (csrc/host_pack.h); the lists are host memory and name atoms of the caller's array. */
int mkamd_ring_interactions_host(mkamd_ctx* ctx, int kind, const float* coords, int64_t n_atoms, int64_t n_frames, const float* box,
                                 const uint32_t* ring_atoms, int64_t n_ring_atoms, const uint32_t* starts1, int64_t n1,
                                 const uint32_t* starts2, const uint32_t* partners, int64_t n2, const float* thresholds,
                                 int64_t* frame_offsets, const uint32_t** pairs, const float** distang);
/* The launch plan of the ring calls (tests, same-box A-B timing).  avoid_mask: 1 not the kernels whose lanes run along frames, 2 not
 * those whose lanes run along the pairs of one frame (default 0: by the shape of the call).  chunk_frames > 0: that many frames per
 * chunk instead of what a 256 MB workspace allows (0: default).  Every plan produces the same lists. */
int mkamd_ctx_set_ring_plan(mkamd_ctx* ctx, int avoid_mask, int64_t chunk_frames);

/* ---- hydrogen bonds of every frame (moleculekit interactions/hbonds/hbonds.pyx: `calculate`) ----
 * The arguments are `calculate`'s:
 *   donors uint32 [n_donors, 2]      (heavy atom, hydrogen) rows; [n_donors, 1] (heavy atoms) with ignore_hs
 *   acceptors uint32 [n_acceptors]
 *   sel1, sel2 uint32 [n_atoms]      per-atom flags.  intra != 0: a pair is tested where sel1[acceptor] != 0 and sel1[heavy] != 0 (sel2 is
 *                                    not read); otherwise where (sel1[acceptor] == 1 and sel2[heavy] == 1) or (sel2[acceptor] == 1 and
 *                                    sel1[heavy] == 1) -- always the donor's HEAVY atom.  A pair whose acceptor IS the heavy atom is skipped
 *   dist_threshold, angle_threshold  A and degrees (the reference's defaults: 2.5, 120); squared / divided by 57.29578 as the reference does
 * box float32 [3, n_frames]: the minimum image is applied per axis only where |d| > box / 2 and box != 0 (a zero axis is open; there is
 * no pbc flag); box NULL: every axis open.  Every float32 operation is the reference's, rounded on its own: the
 * wrapped vector acceptor - hydrogen and its squared length against the threshold (a NaN passes: with ignore_hs a frame of NaN
 * coordinates reports every allowed pair, as the reference does); then heavy - hydrogen, the dot product, the ratio clamped to [-1, 1],
 * the C library's float32 acos restated, reported where the angle is GREATER than the threshold.
 * The work is proportional to the ALLOWED pairs (a donor row is held against the acceptors of the selection its heavy atom is not in),
 * not to n_donors * n_acceptors.
 * Results, the reference's order (frame; donor row; acceptor): frame_offsets int64 [n_frames + 1] (host); *triples int32 [3 n]: heavy
 * atom, hydrogen (-1 with ignore_hs), acceptor.  The list is context-owned (NULL when n = 0) and valid until the next hydrogen-bond call
 * on the context.
 * _dev: coords [n_atoms, 3, n_frames] and box are device pointers and the result list is device memory; the index lists and the flags
 * are HOST arrays in both forms -- they are sorted into classes on the host, once per call, and the kernels never read them (a table of
 * the sorted rows goes up instead).  Every index is checked.  Not asynchronous: the counts reach the host to size the list.
 * MKAMD_EINVAL: a NaN threshold; an atom index >= n_atoms; more than 2^30 frames, donor rows or acceptors; more than 2^31 allowed pairs. */
int mkamd_hbonds_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t n_frames, const float* d_box, const uint32_t* donors,
                     int64_t n_donors, const uint32_t* acceptors, int64_t n_acceptors, const uint32_t* sel1, const uint32_t* sel2,
                     float dist_threshold, float angle_threshold, int intra, int ignore_hs, int64_t* frame_offsets, const int32_t** d_triples);
/* host arrays; only the rows of the donors' and acceptors' atoms are packed and uploaded (csrc/host_pack.h); the list is host memory and
 * names atoms of the caller's array. */
int mkamd_hbonds_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const float* box, const uint32_t* donors,
                      int64_t n_donors, const uint32_t* acceptors, int64_t n_acceptors, const uint32_t* sel1, const uint32_t* sel2,
                      float dist_threshold, float angle_threshold, int intra, int ignore_hs, int64_t* frame_offsets, const int32_t** triples);
/* The launch plan of the hydrogen-bond calls (tests, same-box A-B timing).  avoid_mask: 1 not the kernels whose lanes run along frames,
 * 2 not those whose lanes run along the acceptors of one frame (default 0: by the shape of the call).  chunk_frames > 0: that many frames
 * per chunk instead of what a 256 MB workspace allows (0: default, a multiple of 64).  Every plan produces the same list. */
int mkamd_ctx_set_hbond_plan(mkamd_ctx* ctx, int avoid_mask, int64_t chunk_frames);

/* ---- bond guesser of one frame (moleculekit bondguesser.py: `bond_grid_search`; bondguesser_utils.pyx: the pair test) ----
 *   coords float32 [n_atoms, 3]   one frame, atom-major; must be finite
 *   radii float32 [n_atoms]       the atoms' radii (bondguesser.py's table, the defaults by atom name, 1.5: the caller's)
 *   is_hydrogen uint32 [n_atoms]  != 0: a hydrogen; two hydrogens never bond
 *   grid_cutoff, max_boxes, cutoff_incr   `bond_grid_search`'s (its defaults: 4e6, 1.26): the box side starts at grid_cutoff and is
 *                                 multiplied by cutoff_incr, in double, while the grid has more than max_boxes boxes
 * The grid is the reference's non-periodic one: per-axis float32 minimum, floor(range / float32(box side)) + 1 boxes an axis, an atom's
 * box floor((x - min) / float32(box side)) clipped to the grid -- float32 subtractions and correctly rounded float32 divisions.  A pair
 * of neighbouring boxes' atoms bonds where dist2 = (dx dx + dy dy) + dz dz (every float32 operation rounded on its own) is neither
 * above float32(box side)^2 nor, widened to double, below 0.001, and not above float32(0.6 * double(r_i + r_j))^2.
 * Result: *n rows of *pairs, int32 [n, 2] = (i, j) in the REFERENCE'S ORDER (occupied boxes by their lowest atom; owners ascending; its
 * 14 neighbour relations in its order; partners ascending; rows not sorted within themselves).  The list is context-owned (NULL when
 * n = 0) and valid until the next bond call on the context.  grid (may be NULL) double [4]: boxes per axis and the box side the call
 * settled on.
 * A box may hold at most 4 096 atoms (the cell list's sort and the pair kernels are quadratic in a box's atoms): a frame that puts more
 * into one box -- coincident atoms -- ends the call with MKAMD_EINVAL and a message naming the box and its occupancy.
 * Not asynchronous: the bounds, the occupancies and the size of the list reach the host on the way.
 * MKAMD_EINVAL: a non-finite coordinate; a grid_cutoff that is not positive and finite; max_boxes outside [1, 2^28]; cutoff_incr <= 1;
 * n_atoms >= 2^31; a box over the cap; more than 2^31 bonds.
 * _dev: the three arrays are device pointers and the list is device memory. */
int mkamd_guess_bonds_dev(mkamd_ctx* ctx, const float* d_coords, const float* d_radii, const uint32_t* d_is_hydrogen, int64_t n_atoms,
                          double grid_cutoff, double max_boxes, double cutoff_incr, int64_t* n, const int32_t** d_pairs, double* grid);
/* host arrays; the list is host memory */
int mkamd_guess_bonds_host(mkamd_ctx* ctx, const float* coords, const float* radii, const uint32_t* is_hydrogen, int64_t n_atoms,
                           double grid_cutoff, double max_boxes, double cutoff_incr, int64_t* n, const int32_t** pairs, double* grid);
/* The launch plan of the bond calls (tests, same-box A-B timing).  avoid_mask: 1 not the pair kernels with a thread per owner, 2 not
 * those with a wave per owner (default 0: a wave per owner where some box holds 64 atoms or more).  Both produce the same list. */
int mkamd_ctx_set_bond_plan(mkamd_ctx* ctx, int avoid_mask);

/* ---- steric clashes of one frame (moleculekit distance.py: `find_clashes`) ----
 *   coords float32 [n_atoms, 3]   one frame, atom-major; the selected atoms' must be finite
 *   radii float32 [n_atoms]       the atoms' van der Waals radii (the caller's: the reference's table, 1.7 where it has none)
 *   sel1, sel2 uint32 [n_atoms]   != 0: the atom is in the first / second selection.  self_mode != 0: one selection (sel2 is not read)
 *                                 and rows a < b; otherwise ordered rows (a of sel1, b of sel2) with no such filter, so selections that
 *                                 overlap yield (a, b), (b, a) and (a, a)
 *   ex_start uint32 [n_atoms + 1], ex_partner uint32 [ex_start[n_atoms]]   the exclusion table, or both NULL: row a holds, ascending,
 *                                 the partners b >= a with which (a, b) is excluded.  A row (a, b) with a > b is never looked up (the
 *                                 reference looks rows up as found in a set of (min, max) tuples).  The _dev call trusts the table
 *   overlap                       a clash where dist < float32(float32(r_a + r_b) - float32(overlap)), strictly
 *   cutoff                        the reference's kd-tree radius, 2 max(radii) - overlap over ALL atoms, in double: a row also needs
 *                                 (dx dx + dy dy) + dz dz <= cutoff * cutoff in float64 on the widened coordinates (the kd-tree squares
 *                                 its radius: a negative cutoff searches like its absolute value)
 *   max_boxes                     the cell list's grid holds at most this many boxes (in [1, 2^28]); the box side is at least |cutoff|
 * dist = the correctly rounded float32 root of (dx dx + dy dy) + dz dz, every float32 operation rounded on its own; the row's overlap is
 * float32(float32(r_a + r_b) - dist).
 * Result: *n rows of *pairs int32 [n, 2] = (a, b), *dist float32 [n], *overlap float32 [n].  The lists are context-owned (NULL when
 * n = 0) and valid until the next clash call on the context.  info (may be NULL) double [6]: boxes per axis, the box side, the atoms of
 * the most crowded box, the owners (selected atoms of sel1).
 * _dev: every array is a device pointer, the lists are device memory, and the rows come in the pair kernels' order (owners in cell order,
 * the 27 boxes around each, partners ascending within a box): the same on every run and under both plans; the caller sorts.
 * _host: host arrays, the lists are host memory, sorted by overlap, largest first, equal overlaps by (a, b) ascending; the table is checked.
 * A box may hold at most 4 096 atoms: a frame that puts more into one ends the call with MKAMD_EINVAL and a message naming the box.
 * Not asynchronous.  MKAMD_EINVAL: a non-finite coordinate in a selection; overlap or cutoff not finite; max_boxes outside [1, 2^28];
 * n_atoms >= 2^31; a box over the cap; more than 2^31 rows; (_host) a table that is not a CSR of ascending rows over n_atoms atoms. */
int mkamd_find_clashes_dev(mkamd_ctx* ctx, const float* d_coords, const float* d_radii, const uint32_t* d_sel1, const uint32_t* d_sel2,
                           int64_t n_atoms, int self_mode, const uint32_t* d_ex_start, const uint32_t* d_ex_partner, double overlap, double cutoff,
                           double max_boxes, int64_t* n, const int32_t** d_pairs, const float** d_dist, const float** d_overlap, double* info);
int mkamd_find_clashes_host(mkamd_ctx* ctx, const float* coords, const float* radii, const uint32_t* sel1, const uint32_t* sel2, int64_t n_atoms,
                            int self_mode, const uint32_t* ex_start, const uint32_t* ex_partner, double overlap, double cutoff, double max_boxes,
                            int64_t* n, const int32_t** pairs, const float** dist, const float** overlap_out, double* info);
/* The launch plan of the clash calls (tests, same-box A-B timing).  avoid_mask: 1 not the pair kernels with a thread per owner, 2 not
 * those with a wave per owner (default 0: a wave per owner while the owners number at most 8 192 or some box holds 64 atoms or more).
 * Both produce the same rows in the same order. */
int mkamd_ctx_set_clash_plan(mkamd_ctx* ctx, int avoid_mask);

/* ---- proximity selections over frames (moleculekit atomselect_utils.pyx: `within_distance`, behind `within X of ...`) ----
 *   coords                        _dev: float32 [n_frames][n_atoms][3], frame-major; _host: float32 [n_atoms][3][n_frames], the
 *                                 reference's layout -- only the rows of the atoms sel1 and sel2 name travel
 *   sel1 uint32 [n1]              the queries: atom indices < n_atoms in any order, duplicates allowed (the _dev call trusts them)
 *   sel2 uint32 [n2]              the sources, likewise; may overlap sel1
 *   cutoff                        float32; within where ((dx dx) + dy dy) + dz dz < cutoff * cutoff, strictly, every float32 operation
 *                                 rounded on its own.  Zero, NaN and negative cutoffs, and cutoffs whose square overflows or underflows,
 *                                 behave as that float32 arithmetic says; a NaN anywhere decides "not within"
 *   gate float32 [n_frames][2][3] per frame (min[3], max[3]), or NULL: no gate.  With it a query is looked at only where on some axis
 *                                 x >= min - cutoff or x <= max + cutoff in float32 -- the reference's test, which closes with NaNs and
 *                                 with a negative cutoff
 *   out uint8 [n_frames][n1]      1 where some source is within of the query, 0 otherwise; every element is written
 * The _dev call is asynchronous on the context's stream where it takes the all-pairs kernel (always with n_frames > 1).  One frame
 * with 2 048 sources or more runs over a cell list of the sources, with two round trips; that path is left for the all-pairs kernel, at the same
 * results, where a box would hold more than 4 096 sources, a source coordinate is not finite, the square of the cutoff is not finite
 * or the grid is a single box.  mkamd_ctx_last_dist_kernel names the kernel that decided: "mkamd::k_within_pairs",
 * "mkamd::k_within_cells", or "" where there was nothing to search.
 * MKAMD_EINVAL: a negative size; 2^31 atoms or more; (_host) an index >= n_atoms. */
int mkamd_within_distance_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t n_frames, const uint32_t* d_sel1, int64_t n1,
                              const uint32_t* d_sel2, int64_t n2, float cutoff, const float* d_gate, uint8_t* d_out);
int mkamd_within_distance_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const uint32_t* sel1, int64_t n1,
                               const uint32_t* sel2, int64_t n2, float cutoff, const float* gate, uint8_t* out);
/* The launch plan of the proximity calls (tests, same-box A-B timing).  avoid_mask: 1 not the all-pairs kernel (one frame: the cell list
 * wherever it can run), 2 not the cell list (default 0: the cell list for one frame from 2 048 sources on).  Both give the same bytes. */
int mkamd_ctx_set_within_plan(mkamd_ctx* ctx, int avoid_mask);

/* ---- secondary structure: Kabsch and Sander's DSSP of every frame (moleculekit projections/metricsecondarystructure.py, which
 * hands the frames to an external implementation one at a time).  The rules are stated in DESIGN.md section 19: backbone N-H...O=C
 * energies in float32, every operation rounded once, between residues whose CA atoms are closer than 9 A; the two best acceptors of
 * every donor; n-turns, helices, bends, bridges and ladders with bulge merging.  No box is used. ----
 *   coords float32 [n_atoms][3][n_frames]   the reference's layout, in A; _host: only the rows of the 4 R backbone atoms travel
 *   ca uint32 [R], nco uint32 [R][3]        the CA atom of every residue, and its N, C, O (the _dev call trusts the indices)
 *   proline int32 [R]                       not 0: the residue donates no hydrogen bond
 *   chain int32 [R]                         equal in neighbouring residues: the same chain
 *   simplified                              0: out holds H 3, B 4, E 5, G 6, I 7, T 8, S 9, ' ' 10; else helix 2, strand 1, coil 0
 *   out uint8 [n_frames][R]                 every element is written
 * The _dev call is asynchronous on the context's stream.  The same bytes on every run and under either launch plan;
 * mkamd_ctx_last_dist_kernel names the energy kernel: "mkamd::k_dssp_energy_frames" or "mkamd::k_dssp_energy_atoms".
 * MKAMD_EINVAL: a negative size; 2^30 frames or more; more than 2^18 residues; (_host) an index >= n_atoms. */
int mkamd_dssp_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t n_frames, const uint32_t* d_ca, const uint32_t* d_nco,
                   const int32_t* d_proline, const int32_t* d_chain, int64_t R, int simplified, uint8_t* d_out);
int mkamd_dssp_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const uint32_t* ca, const uint32_t* nco,
                    const int32_t* proline, const int32_t* chain, int64_t R, int simplified, uint8_t* out);
/* The launch plan of the secondary-structure calls (tests, same-box A-B timing).  avoid_mask: 1 not the energy kernel with lanes along
 * frames, 2 not the one with lanes along acceptors (default 0: lanes along acceptors while n_frames * R < 32 768, where the two were measured to cross), 4 chunks of 64 frames whatever
 * the workspace allows.  Every plan gives the same bytes. */
int mkamd_ctx_set_dssp_plan(mkamd_ctx* ctx, int avoid_mask);

#ifdef __cplusplus
}
#endif
#endif /* MKAMD_DISTANCE_H */
