"""The kernel ledger: every kernel instance the compiler emits for the shipped library, tied to the float64 parity modules
that launch it.  Plain data and helpers, no GPU: tests/test_kernel_ledger_cpu.py compares the set in the built object files
with LEDGER | UNCOVERED, the record profiles/kernel_ledger.txt (tools/kernel_coverage.py, from one rocprofv3 kernel trace per
parity module) with LEDGER, and the restatements below of the host arithmetic that selects template instances
(csrc/wino_host.h: nraw, BW, n32; csrc/linhead.hip: ct, ct3) with the library's plan queries.

What the ledger catches: a template instance added or removed without a ledger line (CPU suite).  What it does not: a test
that stops launching a kernel it used to launch -- that shows only when the record is taken again.
The record is per module, not per test: inside a module's own sources a launch by one of its model-level tests counts like a
launch by a kernel-level one.
"""
import glob
import os
import re
import subprocess

import wino_walks as WW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'contrad_amd', 'csrc')
RECORD = os.path.join(ROOT, 'profiles', 'kernel_ledger.txt')
NEVER = 'NEVER'
BY_PLAN_QUERY = 'by plan query'


def normalise(name):
    """A demangled kernel (or ``__device_stub__``) name without ``(anonymous namespace)::``, the ``void`` return type and the
    argument list; namespaces and template arguments are kept, nothing is cut short: ``wino44n::wino44n_kernel<1, 6>``."""
    name = name.strip()
    name = re.sub(r'\s*\[clone [^\]]*\]$', '', name)
    if name.endswith('.kd'):
        name = name[:-3]
    name = name.replace('(anonymous namespace)::', '').replace('__device_stub__', '')
    if name.startswith('void '):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):              # the argument list opens at the first '(' outside the template arguments
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            name = name[:i]
            break
    return re.sub(r'\s*,\s*', ', ', name.strip())


def shipped_objects():
    """The object files of libcontrad_hip.so (build.py: one per csrc/*.hip)."""
    return [s[:-4] + '.o' for s in sorted(glob.glob(os.path.join(CSRC, '*.hip')))]


def dev_objects():
    """The object files of libcontrad_hip_dev.so: igemm_dev.o in place of igemm.o (build.py: DEV_SOURCES)."""
    from contrad_amd.build import DEV_SOURCES
    return [o[:-2] + '_dev.o' if os.path.basename(o)[:-2] in DEV_SOURCES else o for o in shipped_objects()]


def instance_sources(objects=None):
    """{kernel instance: source name ('igemm', 'linhead', ...)} of the object files: the host-side ``__device_stub__`` symbols
    (local ones included: the kernels live in anonymous namespaces) as ``nm -C`` prints them, normalised."""
    found = {}
    for o in (shipped_objects() if objects is None else objects):
        out = subprocess.run(['nm', '-C', o], check=True, capture_output=True, text=True).stdout
        src = os.path.basename(o)[:-2]
        src = src[:-4] if src.endswith('_dev') else src
        for line in out.splitlines():
            if '__device_stub__' in line:
                inst = normalise(line.split(None, 2)[2])
                assert found.setdefault(inst, src) == src, (inst, src)          # one source per instance
    return found


def compiled_instances(objects=None):
    """The set of kernel instances in the object files (default: the shipped library's)."""
    return set(instance_sources(objects))


# module: (the csrc sources whose kernels it is a parity module for, why it qualifies).  A module counts if, for every kernel it
# launches from these sources, it compares the whole output with a float64 (or exact integer) restatement that uses none of this
# project's kernels.  Several of these modules also hold whole-model, training-loop and command-line tests, which launch kernels
# of other sources (conv, augmentation, optimizer): those launches are in the module's trace and count for nothing -- the record
# and the ledger credit a module only inside its sources.  Left out: test_filter_prep_gpu (compares prepared filters bitwise with
# the per-call transform, a kernel of this project) and test_augment_edge_gpu (compares with recorded fp32 fixtures).
_CONV = 'whole output tensors against the float64 im2col GEMM of tests/conv_ref64.py, NaN guard bands'
PARITY_MODULES = {
    'test_conv_paths_gpu': (('igemm',), 'every planned conv path and the forced Winograd instances: ' + _CONV),
    'test_igemm_forms_gpu': (('igemm',), 'every tile, split and block-order form of the direct conv kernels: ' + _CONV),
    'test_wino_walks_gpu': (('igemm',), 'the persistent item walks of the Winograd kernels: ' + _CONV),
    'test_wgrad_staging_gpu': (('igemm',), 'the Winograd weight gradients on the forced entry point: ' + _CONV),
    'test_dstep_kernels_gpu': (('ntxent', 'specnorm', 'conv_small', 'elementwise'),
                               'every launch form against tests/dstep_ref64.py (plain float64 torch), whole tensors, guard storage'),
    'test_augment_kernels_gpu': (('augment',), 'every launch form against tests/aug_ref64.py (plain float64 torch), guard storage'),
    'test_sg2_ops_kernels_gpu': (('stylegan2_ops',), 'every launch form against tests/sg2_ref64.py (plain float64 torch), guard storage'),
    'test_autograd_nodes_gpu': (('igemm', 'conv_small', 'elementwise', 'stylegan2_ops', 'specnorm'),
                                'every node output and first / second derivative, whole tensors, against its float64 twin '
                                '(tests/nodes_ref64.py)'),
    'test_gp_kernels_gpu': (('gp',), 'every launch form against tests/gp_ref64.py (float64), guard storage'),
    'test_baselines_gpu': (('baseline_aug',), 'the kernel tests compare with tests/baselines_ref64.py (float64), guard storage'),
    'test_cddls_gpu': (('cddls',), 'every kernel alone against float64 with explicit noise (tests/cddls_ref64.py)'),
    'test_linhead_gpu': (('linhead',), 'every tensor of an iteration against tests/linhead_ref64.py (float64), guard storage'),
    'test_knn_gpu': (('knn',), 'the select-and-vote kernel on a given S against tests/knn_ref64.py (float64)'),
    'test_prdc_gpu': (('prdc',), 'both kernels on a given S against tests/prdc_ref64.py: exact integer counts'),
    'test_kid_gpu': (('kid',), 'the sum kernel on a given S against math.fsum of the float64 terms (tests/kid_ref64.py)'),
    'test_data_gpu': (('data',), 'the uint8 gather bitwise against ToTensor on the host'),
    'test_imagegrid_gpu': (('imagegrid',), 'byte outputs compared exactly with tests/grid_ref.py'),
    'test_far_offsets_gpu': (('igemm', 'stylegan2_ops', 'conv_small', 'elementwise', 'data', 'linhead'),
                             'operands spanning more than 2^32 bytes against float64 over the whole output'),
}


def credited(module, source):
    """Does a launch by ``module`` of a kernel from csrc/<source>.hip count?"""
    return source in PARITY_MODULES[module][0]


# ---------------------------------------------------------------------------------------------------------------------------
# Host arithmetic that selects template instances, restated

def cdiv(a, b):
    return -(-a // b)


def linhead_plan(N, K, C):
    """linhead_plan of csrc/linhead.hip: (K-splits, classes per thread of the logits kernel, 64-row tiles, classes per
    thread of the weight-gradient kernel)."""
    ct, ct3, row_tiles = cdiv(C, 16), cdiv(C, 32), cdiv(N, 64)
    nchunks = cdiv(K, 64)
    want = min(cdiv(512, row_tiles), max(K // (16 * ct), 1), nchunks)
    cps = cdiv(nchunks, want)
    return cdiv(nchunks, cps), ct, row_tiles, ct3


def linhead_instances(N, K, C):
    """The two template instances one training iteration of the head launches at (N, K, C)."""
    _S, ct, _rt, ct3 = linhead_plan(N, K, C)
    return 'linhead_logits_kernel<%d>' % ct, 'linhead_wgrad_kernel<%d>' % ct3


def wino_instance(desc, mode, f44=True):
    """The forward (mode 0) / data-gradient (mode 1) kernel instance a Winograd launch of the layer runs.  ``desc`` =
    (N, H, W, C, K, k, stride, pad): the layer's input map and input / output channels in both modes.  The family follows from
    the filter (4x4 stride 2: wino22; 3x3 stride 2 pad 0: wino23; 3x3 stride 1: F(4x4,3x3) when ``f44`` -- the 64-wide
    wino44 or the 32-wide wino44n by Wino44::n32 -- else F(2x2,3x3), which has one instance per mode); the instance inside
    the family from Wino22::launch / Wino23::launch (nraw) and Wino44::launch (BW).  None: no family takes the filter."""
    N, H, W, C, K, k, s, p = desc
    cout = K if mode == 0 else C
    if (k, s, p) == (4, 2, 1):
        GH, GW = H // 2, W // 2
        nimg = 128 // ((GH // 2) * (GW // 2))
        nraw = cdiv(2 * nimg * (GH + 1) * (GW + 1), 256)
        return 'wino22::wino22_kernel<%d, %d>' % (mode, min(max(nraw, 5), 7))
    if (k, s, p) == (3, 2, 0) and mode == 0:
        Ho, Wo = (H - 1) // 2, (W - 1) // 2
        TW, TH = (16, 8) if Wo >= 32 else (Wo // 2, Ho // 2)
        nimg = 128 // (TH * TW)
        nraw = cdiv(2 * nimg * (2 * TH + 1) * (2 * TW + 1), 256)
        return 'wino23::wino23_kernel<%d>' % min(max(nraw, 5), 7)
    if (k, s, p) == (3, 1, 1):
        if not f44:
            return 'wino::wino_kernel<%d>' % mode
        TW, TH = min(8, W // 4), min(4, H // 4)
        patches = cdiv(N, 32 // (TH * TW)) * (H // (4 * TH)) * (W // (4 * TW))
        BW = 4 * TW + 2
        if WW.n32(cout, W, patches):
            return 'wino44n::wino44n_kernel<%d, %d>' % (mode, BW)
        return 'wino44::wino44_kernel<%d, %d>' % (mode, BW)
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# The ledger (from the record: tools/kernel_coverage.py --ledger)

# instance: the parity modules that launch it (inside their sources)
LEDGER = {
    'adam_kernel': ['test_dstep_kernels_gpu'],
    'axpby_kernel': ['test_dstep_kernels_gpu', 'test_far_offsets_gpu'],
    'blur_adj_kernel': ['test_augment_kernels_gpu'],
    'blur_h_kernel': ['test_augment_kernels_gpu'],
    'blur_v_kernel': ['test_augment_kernels_gpu'],
    'bn_relu_apply_kernel': ['test_dstep_kernels_gpu', 'test_far_offsets_gpu'],
    'bn_relu_bwd_apply_kernel': ['test_dstep_kernels_gpu', 'test_far_offsets_gpu'],
    'bn_relu_bwd_stats_kernel': ['test_dstep_kernels_gpu', 'test_far_offsets_gpu'],
    'bn_running_update_kernel': ['test_dstep_kernels_gpu'],
    'bn_stats_reduce_update_kernel': ['test_far_offsets_gpu'],
    'cddls_bn_relu_bwd_eval_kernel': ['test_cddls_gpu'],
    'cddls_compose_kernel': ['test_cddls_gpu'],
    'cddls_energy_kernel': ['test_cddls_gpu'],
    'cddls_feature_seed_kernel': ['test_cddls_gpu'],
    'cddls_image_end_kernel': ['test_cddls_gpu'],
    'cddls_latent_update_kernel': ['test_cddls_gpu'],
    'cddls_normal_fill_kernel': ['test_cddls_gpu'],
    'colstats_partial_kernel<false>': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'colstats_partial_kernel<true>': ['test_dstep_kernels_gpu'],
    'colstats_partial_vec_kernel<false, 128>': ['test_dstep_kernels_gpu'],
    'colstats_partial_vec_kernel<false, 16>': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'colstats_partial_vec_kernel<false, 256>': ['test_dstep_kernels_gpu'],
    'colstats_partial_vec_kernel<false, 32>': ['test_dstep_kernels_gpu'],
    'colstats_partial_vec_kernel<false, 64>': ['test_dstep_kernels_gpu'],
    'colstats_partial_vec_kernel<true, 128>': ['test_dstep_kernels_gpu'],
    'colstats_partial_vec_kernel<true, 16>': ['test_dstep_kernels_gpu', 'test_far_offsets_gpu'],
    'colstats_partial_vec_kernel<true, 256>': ['test_dstep_kernels_gpu'],
    'colstats_partial_vec_kernel<true, 32>': ['test_dstep_kernels_gpu'],
    'colstats_partial_vec_kernel<true, 64>': ['test_dstep_kernels_gpu'],
    'colstats_reduce_kernel': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'consistency_kernel': ['test_baselines_gpu'],
    'contrast_bwd_kernel<128>': ['test_dstep_kernels_gpu'],
    'contrast_bwd_kernel<256>': ['test_dstep_kernels_gpu'],
    'contrast_bwd_kernel<64>': ['test_dstep_kernels_gpu'],
    'contrast_bwd_reduce_kernel': ['test_dstep_kernels_gpu'],
    'contrast_fwd_kernel<128>': ['test_dstep_kernels_gpu'],
    'contrast_fwd_kernel<256>': ['test_dstep_kernels_gpu'],
    'contrast_fwd_kernel<64>': ['test_dstep_kernels_gpu'],
    'contrast_loss_reduce_kernel': ['test_dstep_kernels_gpu'],
    'conv_c32_kernel<0>': ['test_conv_paths_gpu', 'test_far_offsets_gpu'],
    'conv_c32_kernel<1>': ['test_conv_paths_gpu', 'test_far_offsets_gpu'],
    'cutout_kernel': ['test_augment_kernels_gpu'],
    'dgrad_reduce_kernel': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'diffaug_apply_kernel<false>': ['test_baselines_gpu'],
    'diffaug_apply_kernel<true>': ['test_baselines_gpu'],
    'diffaug_bwd_apply_kernel<false>': ['test_baselines_gpu'],
    'diffaug_bwd_apply_kernel<true>': ['test_baselines_gpu'],
    'diffaug_bwd_sum_kernel': ['test_baselines_gpu'],
    'diffaug_small_bwd_kernel<false>': ['test_baselines_gpu'],
    'diffaug_small_bwd_kernel<true>': ['test_baselines_gpu'],
    'diffaug_small_kernel<false>': ['test_baselines_gpu'],
    'diffaug_small_kernel<true>': ['test_baselines_gpu'],
    'diffaug_sum_kernel<false>': ['test_baselines_gpu'],
    'diffaug_sum_kernel<true>': ['test_baselines_gpu'],
    'filter_prep_kernel': ['test_far_offsets_gpu'],
    'fused_bias_act_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'fwd_k1_kernel': ['test_conv_paths_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'fwd_reduce_kernel': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'gan_d_loss_2n_kernel': ['test_baselines_gpu'],
    'gan_d_loss_kernel': ['test_dstep_kernels_gpu'],
    'gan_g_loss_kernel': ['test_dstep_kernels_gpu'],
    'gather_u8_nchw_kernel<false>': ['test_data_gpu'],
    'gather_u8_nchw_kernel<true>': ['test_data_gpu', 'test_far_offsets_gpu'],
    'gp_interpolate_kernel': ['test_gp_kernels_gpu'],
    'gp_penalty_apply_kernel': ['test_gp_kernels_gpu'],
    'gp_penalty_small_kernel': ['test_gp_kernels_gpu'],
    'gp_penalty_sum_kernel': ['test_gp_kernels_gpu'],
    'gp_penalty_value_kernel': ['test_gp_kernels_gpu'],
    'hfrt_bwd_kernel': ['test_baselines_gpu'],
    'hfrt_fwd_kernel<false>': ['test_baselines_gpu'],
    'hfrt_fwd_kernel<true>': ['test_baselines_gpu'],
    'igemm_kernel<0, 128, 128, true>': ['test_igemm_forms_gpu'],
    'igemm_kernel<0, 128, 64, true>': ['test_igemm_forms_gpu', 'test_far_offsets_gpu'],
    'igemm_kernel<0, 64, 128, true>': ['test_igemm_forms_gpu'],
    'igemm_kernel<0, 64, 64, false>': ['test_conv_paths_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_kernel<0, 64, 64, true>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu'],
    'igemm_kernel<1, 128, 128, true>': ['test_igemm_forms_gpu', 'test_far_offsets_gpu'],
    'igemm_kernel<1, 128, 64, true>': ['test_igemm_forms_gpu', 'test_far_offsets_gpu'],
    'igemm_kernel<1, 64, 128, true>': ['test_igemm_forms_gpu'],
    'igemm_kernel<1, 64, 64, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_kernel<1, 64, 64, true>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu'],
    'igemm_kernel<2, 128, 128, true>': ['test_igemm_forms_gpu'],
    'igemm_kernel<2, 128, 64, true>': ['test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_kernel<2, 64, 128, true>': ['test_igemm_forms_gpu'],
    'igemm_kernel<2, 64, 64, false>': ['test_conv_paths_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_kernel<2, 64, 64, true>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<0, 128, 128, false>': ['test_igemm_forms_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<0, 128, 32, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<0, 128, 64, false>': ['test_igemm_forms_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<0, 64, 128, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu'],
    'igemm_lean_kernel<0, 64, 64, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<1, 128, 128, false>': ['test_igemm_forms_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<1, 128, 128, true>': ['test_igemm_forms_gpu'],
    'igemm_lean_kernel<1, 128, 32, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu'],
    'igemm_lean_kernel<1, 128, 32, true>': ['test_far_offsets_gpu'],
    'igemm_lean_kernel<1, 128, 64, false>': ['test_igemm_forms_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<1, 128, 64, true>': ['test_igemm_forms_gpu'],
    'igemm_lean_kernel<1, 64, 128, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu'],
    'igemm_lean_kernel<1, 64, 128, true>': ['test_igemm_forms_gpu'],
    'igemm_lean_kernel<1, 64, 64, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<1, 64, 64, true>': ['test_igemm_forms_gpu'],
    'igemm_lean_kernel<2, 128, 128, false>': ['test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<2, 128, 32, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'igemm_lean_kernel<2, 128, 64, false>': ['test_igemm_forms_gpu'],
    'igemm_lean_kernel<2, 64, 128, false>': ['test_igemm_forms_gpu'],
    'igemm_lean_kernel<2, 64, 64, false>': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_autograd_nodes_gpu'],
    'image_grid_u8_kernel': ['test_imagegrid_gpu'],
    'kid_final_kernel': ['test_kid_gpu'],
    'kid_sums_kernel': ['test_kid_gpu'],
    'knn_select_kernel': ['test_knn_gpu'],
    'l2norm_bwd_kernel': ['test_dstep_kernels_gpu'],
    'l2norm_fwd_kernel': ['test_dstep_kernels_gpu'],
    'lincomb_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'linhead_logits_kernel<1>': ['test_linhead_gpu', 'test_far_offsets_gpu'],
    'linhead_logits_kernel<2>': ['test_linhead_gpu'],
    'linhead_logits_kernel<3>': ['test_linhead_gpu'],
    'linhead_logits_kernel<4>': ['test_linhead_gpu'],
    'linhead_logits_kernel<5>': ['test_linhead_gpu'],
    'linhead_logits_kernel<6>': ['test_linhead_gpu'],
    'linhead_logits_kernel<7>': ['test_linhead_gpu'],
    'linhead_logits_kernel<8>': ['test_linhead_gpu'],
    'linhead_loss_kernel': ['test_linhead_gpu', 'test_far_offsets_gpu'],
    'linhead_wgrad_kernel<1>': ['test_linhead_gpu', 'test_far_offsets_gpu'],
    'linhead_wgrad_kernel<2>': ['test_linhead_gpu'],
    'linhead_wgrad_kernel<3>': ['test_linhead_gpu'],
    'linhead_wgrad_kernel<4>': ['test_linhead_gpu'],
    'mbstd_kernel<0>': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu'],
    'mbstd_kernel<1>': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu'],
    'mbstd_kernel<2>': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu'],
    'modconv_demod_kernel': ['test_sg2_ops_kernels_gpu'],
    'modconv_epilogue_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'modconv_tables_kernel': ['test_sg2_ops_kernels_gpu'],
    'nhwc_dot_final_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'nhwc_dot_partial_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'nhwc_scale_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'pixelnorm_kernel': ['test_sg2_ops_kernels_gpu'],
    'prdc_count_kernel<false, true>': ['test_prdc_gpu'],
    'prdc_count_kernel<true, false>': ['test_prdc_gpu'],
    'prdc_count_kernel<true, true>': ['test_prdc_gpu'],
    'prdc_kth_kernel': ['test_prdc_gpu'],
    'pull_kernel': ['test_dstep_kernels_gpu'],
    'rgb_conv_dgrad_kernel<1, 1>': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'rgb_conv_dgrad_kernel<1, 2>': ['test_dstep_kernels_gpu'],
    'rgb_conv_dgrad_kernel<3, 1>': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'rgb_conv_fwd_kernel<1, 3>': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'rgb_conv_fwd_kernel<3, 3>': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'rgb_conv_wgrad_kernel<1, 3>': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'rgb_conv_wgrad_kernel<3, 3>': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'rgb_dgrad3_tile_kernel': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'rgb_wgrad_reduce_kernel': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'scale_dev_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'simclr_apply_kernel': ['test_augment_kernels_gpu'],
    'simclr_bwd_gather_x_kernel': ['test_augment_kernels_gpu'],
    'simclr_bwd_gather_y_kernel': ['test_augment_kernels_gpu'],
    'simclr_bwd_gm_kernel': ['test_augment_kernels_gpu'],
    'simclr_small_bwd_kernel': ['test_augment_kernels_gpu'],
    'simclr_small_kernel': ['test_augment_kernels_gpu'],
    'simclr_stats_kernel': ['test_augment_kernels_gpu'],
    'sn_bwd_dot_kernel': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'sn_bwd_write_kernel': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'sn_phase1_kernel': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'sn_phase2_kernel': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'sn_phase3_kernel': ['test_dstep_kernels_gpu', 'test_autograd_nodes_gpu'],
    'sumsq_final_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'sumsq_partial_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'upfirdn2d_kernel<1>': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu'],
    'upfirdn2d_kernel<4>': ['test_sg2_ops_kernels_gpu'],
    'upfirdn2d_strip_kernel<4>': ['test_sg2_ops_kernels_gpu'],
    'upfirdn4_u1d1_buf_kernel<2>': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'upfirdn4_u1d1_kernel': ['test_sg2_ops_kernels_gpu', 'test_far_offsets_gpu'],
    'upfirdn4_u1d2_buf_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'upfirdn4_u1d2_kernel': ['test_sg2_ops_kernels_gpu', 'test_far_offsets_gpu'],
    'upfirdn4_u2d1_buf_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'upfirdn4_u2d1_kernel': ['test_sg2_ops_kernels_gpu', 'test_far_offsets_gpu'],
    'upfirdn4_u2d1_planes_kernel': ['test_sg2_ops_kernels_gpu', 'test_autograd_nodes_gpu'],
    'wgrad_c32_kernel': ['test_conv_paths_gpu', 'test_far_offsets_gpu'],
    'wgrad_reduce_kernel': ['test_conv_paths_gpu', 'test_igemm_forms_gpu', 'test_wgrad_staging_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino22::wino22_filter_kernel<0>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_far_offsets_gpu'],
    'wino22::wino22_filter_kernel<1>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino22::wino22_kernel<0, 5>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_far_offsets_gpu'],
    'wino22::wino22_kernel<0, 6>': ['test_wino_walks_gpu'],
    'wino22::wino22_kernel<0, 7>': ['test_wino_walks_gpu'],
    'wino22::wino22_kernel<1, 5>': ['test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino22::wino22_kernel<1, 6>': ['test_conv_paths_gpu', 'test_wino_walks_gpu'],
    'wino22::wino22_kernel<1, 7>': ['test_wino_walks_gpu'],
    'wino22::wino22_wgrad_kernel': ['test_conv_paths_gpu', 'test_wgrad_staging_gpu', 'test_far_offsets_gpu'],
    'wino23::wino23_filter_kernel': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_far_offsets_gpu'],
    'wino23::wino23_kernel<5>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_far_offsets_gpu'],
    'wino23::wino23_kernel<6>': ['test_wino_walks_gpu'],
    'wino23::wino23_kernel<7>': ['test_wino_walks_gpu'],
    'wino44::wino44_filter_kernel<0>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino44::wino44_filter_kernel<1>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino44::wino44_kernel<0, 10>': ['test_conv_paths_gpu', 'test_wino_walks_gpu'],
    'wino44::wino44_kernel<0, 18>': ['test_wino_walks_gpu'],
    'wino44::wino44_kernel<0, 34>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_far_offsets_gpu'],
    'wino44::wino44_kernel<1, 10>': ['test_wino_walks_gpu'],
    'wino44::wino44_kernel<1, 18>': ['test_wino_walks_gpu'],
    'wino44::wino44_kernel<1, 34>': ['test_conv_paths_gpu', 'test_far_offsets_gpu'],
    'wino44n::wino44n_kernel<0, 10>': ['test_wino_walks_gpu'],
    'wino44n::wino44n_kernel<0, 18>': ['test_wino_walks_gpu'],
    'wino44n::wino44n_kernel<0, 34>': ['test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino44n::wino44n_kernel<0, 6>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_far_offsets_gpu'],
    'wino44n::wino44n_kernel<1, 10>': ['test_conv_paths_gpu'],
    'wino44n::wino44n_kernel<1, 18>': ['test_wino_walks_gpu'],
    'wino44n::wino44n_kernel<1, 34>': ['test_conv_paths_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino44n::wino44n_kernel<1, 6>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_far_offsets_gpu'],
    'wino::wino_filter_kernel<0>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino::wino_filter_kernel<1>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino::wino_kernel<0>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino::wino_kernel<1>': ['test_conv_paths_gpu', 'test_wino_walks_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
    'wino::wino_wgrad_kernel': ['test_conv_paths_gpu', 'test_wgrad_staging_gpu', 'test_autograd_nodes_gpu', 'test_far_offsets_gpu'],
}

# Meant to be empty: instance -> why no parity module launches it.  tests/test_kernel_ledger_cpu.py pins the set.
UNCOVERED = {}

# Instances the host picks by arithmetic no plan query reports: instance -> (parity module, case table, case id) of the smallest
# case that selects it; the id carries the geometry (walks / paths: images x H x W x C - K, filter; linhead: N x K x C x ...).
HOST_SELECTED = {
    'linhead_logits_kernel<1>': ('test_linhead_gpu', 'CASES', '70x200x3x0x0x2.0'),
    'linhead_logits_kernel<2>': ('test_linhead_gpu', 'CASES', '70x200x20x0x0x2.0'),
    'linhead_logits_kernel<3>': ('test_linhead_gpu', 'CASES', '70x200x40x0x0x2.0'),
    'linhead_logits_kernel<4>': ('test_linhead_gpu', 'CASES', '70x200x64x0x0x2.0'),
    'linhead_logits_kernel<5>': ('test_linhead_gpu', 'CASES', '70x200x72x3x1x2.0'),
    'linhead_logits_kernel<6>': ('test_linhead_gpu', 'CASES', '70x200x96x0x0x2.0'),
    'linhead_logits_kernel<7>': ('test_linhead_gpu', 'CASES', '250x512x100x0x0x2.0'),
    'linhead_logits_kernel<8>': ('test_linhead_gpu', 'CASES', '5x8192x128x0x0x2.0'),
    'linhead_wgrad_kernel<1>': ('test_linhead_gpu', 'CASES', '70x200x3x0x0x2.0'),
    'linhead_wgrad_kernel<2>': ('test_linhead_gpu', 'CASES', '70x200x64x0x0x2.0'),
    'linhead_wgrad_kernel<3>': ('test_linhead_gpu', 'CASES', '70x200x96x0x0x2.0'),
    'linhead_wgrad_kernel<4>': ('test_linhead_gpu', 'CASES', '5x8192x128x0x0x2.0'),
    'wino22::wino22_kernel<0, 5>': ('test_conv_paths_gpu', 'PATH_CASES', 'p8-m0-48x32x32x8-512-k4s2p1'),
    'wino22::wino22_kernel<0, 6>': ('test_wino_walks_gpu', 'WALK_CASES', 'p8-m0-1645x16x16x8-192-k4s2p1'),
    'wino22::wino22_kernel<0, 7>': ('test_wino_walks_gpu', 'WALK_CASES', 'p8-m0-6583x8x8x8-192-k4s2p1'),
    'wino22::wino22_kernel<1, 5>': ('test_wino_walks_gpu', 'WALK_CASES', 'p8-m1-103x32x32x192-16-k4s2p1'),
    'wino22::wino22_kernel<1, 6>': ('test_conv_paths_gpu', 'PATH_CASES', 'p8-m1-48x16x16x512-32-k4s2p1'),
    'wino22::wino22_kernel<1, 7>': ('test_wino_walks_gpu', 'WALK_CASES', 'p8-m1-1655x8x8x192-16-k4s2p1'),
    'wino23::wino23_kernel<5>': ('test_conv_paths_gpu', 'PATH_CASES', 'p10-m0-192x33x33x16-256-k3s2p0'),
    'wino23::wino23_kernel<6>': ('test_wino_walks_gpu', 'WALK_CASES', 'p10-m0-1493x17x17x16-192-k3s2p0'),
    'wino23::wino23_kernel<7>': ('test_wino_walks_gpu', 'WALK_CASES', 'p10-m0-5977x9x9x16-192-k3s2p0'),
    'wino44::wino44_kernel<0, 10>': ('test_conv_paths_gpu', 'PATH_CASES', 'p9-m0-229x8x8x32-512-k3s1p1'),
    'wino44::wino44_kernel<0, 18>': ('test_wino_walks_gpu', 'WALK_CASES', 'p9-m0-373x16x16x32-192-k3s1p1'),
    'wino44::wino44_kernel<0, 34>': ('test_conv_paths_gpu', 'PATH_CASES', 'p9-m0-16x32x32x32-512-k3s1p1'),
    'wino44::wino44_kernel<1, 10>': ('test_wino_walks_gpu', 'WALK_CASES', 'p9-m1-1493x8x8x192-32-k3s1p1'),
    'wino44::wino44_kernel<1, 18>': ('test_wino_walks_gpu', 'WALK_CASES', 'p9-m1-373x16x16x192-32-k3s1p1'),
    'wino44::wino44_kernel<1, 34>': ('test_conv_paths_gpu', 'PATH_CASES', 'p9-m1-16x32x32x512-32-k3s1p1'),
    'wino44n::wino44n_kernel<0, 10>': ('test_wino_walks_gpu', 'WALK_CASES', 'p11-m0-1493x8x8x32-96-k3s1p1'),
    'wino44n::wino44n_kernel<0, 18>': ('test_wino_walks_gpu', 'WALK_CASES', 'p11-m0-373x16x16x32-96-k3s1p1'),
    'wino44n::wino44n_kernel<0, 34>': ('test_wino_walks_gpu', 'WALK_CASES', 'p11-m0-94x32x32x32-96-k3s1p1'),
    'wino44n::wino44n_kernel<0, 6>': ('test_conv_paths_gpu', 'PATH_CASES', 'p11-m0-1536x4x4x32-160-k3s1p1'),
    'wino44n::wino44n_kernel<1, 10>': ('test_conv_paths_gpu', 'INSTANCE_CASES', 'wino44n::wino44n_kernel<1, 10>'),
    'wino44n::wino44n_kernel<1, 18>': ('test_wino_walks_gpu', 'WALK_CASES', 'p11-m1-373x16x16x96-32-k3s1p1'),
    'wino44n::wino44n_kernel<1, 34>': ('test_conv_paths_gpu', 'INSTANCE_CASES', 'wino44n::wino44n_kernel<1, 34>'),
    'wino44n::wino44n_kernel<1, 6>': ('test_conv_paths_gpu', 'PATH_CASES', 'p11-m1-1536x4x4x160-32-k3s1p1'),
}


# ---------------------------------------------------------------------------------------------------------------------------
# The record

def read_record(path=RECORD):
    """profiles/kernel_ledger.txt as {instance: {module: count or 'by plan query'}} ({}: NEVER)."""
    rec = {}
    with open(path) as f:
        for line in f:
            if line.startswith('#') or not line.strip():
                continue
            fields = line.rstrip('\n').split('\t')
            inst, rest = fields[0], fields[1:]
            rec[inst] = {}
            if rest == [NEVER]:
                continue
            for item in rest:
                module, count = item.split('=', 1)
                rec[inst][module] = count if count == BY_PLAN_QUERY else int(count)
    return rec
