// mk_affine.h -- the per-item rigid transform x' = float32(M x + t), evaluated in double.
//
// One expression shared by every place that applies an affine of the [12] layout of include/mkamd_voxel.h (3b) -- the
// binning and exact fix-up sites of kernels.h and the alignment kernels of align_kernels.h -- so that coordinates aligned
// by k_align_apply and then voxelized are bit for bit the coordinates the voxelizer computes when it is handed the same
// affine.  Plain C++ on doubles: it compiles unchanged against mk_device.h and against the test emulator's device header.
#pragma once

// A: row-major 3x3 matrix M, then the translation t (A[9..11]); xyz: float[3], transformed in place.  The operation order is part
// of the contract: the voxelizer's results depend on it bit for bit.  (A macro rather than an inline function: the call sites in
// kernels.h then compile to exactly the instructions they compiled to before the expression was shared -- an always-inline
// function reached the same arithmetic, but the scheduler placed two waits / nops of the exact fix-up kernels differently.)
#define MK_AFFINE_APPLY(A_, xyz_)                                                                             \
    do {                                                                                                        \
        const double* mk_A_ = (A_);                                                                             \
        const double mk_x_ = (double)(xyz_)[0], mk_y_ = (double)(xyz_)[1], mk_z_ = (double)(xyz_)[2];           \
        (xyz_)[0] = (float)(mk_A_[0] * mk_x_ + mk_A_[1] * mk_y_ + mk_A_[2] * mk_z_ + mk_A_[9]);                 \
        (xyz_)[1] = (float)(mk_A_[3] * mk_x_ + mk_A_[4] * mk_y_ + mk_A_[5] * mk_z_ + mk_A_[10]);                \
        (xyz_)[2] = (float)(mk_A_[6] * mk_x_ + mk_A_[7] * mk_y_ + mk_A_[8] * mk_z_ + mk_A_[11]);                \
    } while (0)
