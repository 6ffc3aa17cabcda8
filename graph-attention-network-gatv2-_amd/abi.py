"""ctypes binding of ``include/gatv2_abi.h`` (libgatv2_hip.so) — the Python host side.

This is the same seam the C++ ``train_edge`` host uses; Python is here for tests, the benchmark
and ``torch.distributed`` plumbing.  There is NO CPU fallback: if the HIP library is missing or
fails to load, importing callers get a loud ``GatLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgatv2_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "gatv2_abi.h"))


class GatLibraryError(RuntimeError):
    pass


class GatError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[gat status {code}] {msg}")
        self.code = code


class _Config(C.Structure):
    _fields_ = [
        ("num_layers", C.c_int32),
        ("heads", C.POINTER(C.c_int32)),
        ("outdims", C.POINTER(C.c_int32)),
        ("in_dim", C.c_int32),
        ("num_classes", C.c_int32),
        ("negative_slope", C.c_float),
        ("device", C.c_int32),
        ("stream", C.c_void_p),
        ("flat_lrelu_index", C.c_int32),
        ("collect_timing", C.c_int32),
        ("keep_taps", C.c_int32),
        ("storage_dtype", C.c_int32),
    ]


class _OptimizerConfig(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("flags", C.c_int32),
        ("lr", C.c_float), ("momentum", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("weight_decay", C.c_float),
        ("decay_groups", C.c_uint32),
        ("clip_mode", C.c_int32), ("clip_threshold", C.c_float),
    ]


# enums of the header
PARAM_W, PARAM_A, PARAM_WO, PARAM_WRES, PARAM_B = 0, 1, 2, 3, 4
PARAM_LN_G, PARAM_LN_B = 5, 6
PARAM_WE = 7                                # edge features (set_edge_dim): flat [l][H_l*D_l][Fe], behind the others
PARAM_GROUPS = (PARAM_W, PARAM_A, PARAM_WO, PARAM_WRES, PARAM_B, PARAM_LN_G, PARAM_LN_B, PARAM_WE)      # the packed order
PARAM_HEAD_W, PARAM_HEAD_B = 8, 9           # hidden layer in front of the head (set_head_hidden): W1 [Dh][D_last], b1 [Dh], behind PARAM_WE
PARAM_GROUPS_ALL = PARAM_GROUPS + (PARAM_HEAD_W, PARAM_HEAD_B)         # the packed order of a context with a hidden head layer
HEAD_ACT_LRELU = 1
HEAD_ACTS = {"relu": 0, "lrelu": HEAD_ACT_LRELU}
EDGE_DIM_MAX = 64
RES_LINEAR, RES_BIAS = 1, 2
NORM_LAYER, NORM_SKIP_LAST = 1, 2
PARAM_NORM_G, PARAM_NORM_B = PARAM_LN_G, PARAM_LN_B       # the same two groups, as a batch-norm context reads them (set_batch_norm)
BN_ON, BN_SKIP_LAST = 1, 2
BN_RUNNING_MEAN, BN_RUNNING_VAR, BN_BATCH_MEAN, BN_BATCH_RSTD = 0, 1, 2, 3
TABLE_PL, TABLE_GPL = 0, 1
COMM_GPL_BF16 = 1
COMM_PIPELINE = 2
COMM_HALO = 3
(TAP_SRC, TAP_DST, TAP_ALPHA, TAP_HPRE, TAP_HOUT, TAP_Y, TAP_G, TAP_GE, TAP_MAX, TAP_SUM, TAP_PL,
 TAP_PR, TAP_SCORE, TAP_GALPHA, TAP_GX) = range(15)
TAP_ATTN_KEEP, TAP_FEAT_KEEP = 15, 16       # dropout factors (0 or 1/(1-p)) for the step the counter holds
TAP_EDGE_KEEP = 17                          # DropEdge: 1 = edge kept, 0 = dropped, [E], likewise
TAP_POOLED = 18                             # readout: the pooled rows the head reads, [n_graphs][D_last] (last layer)
DROPEDGE_KEEP_SELF, DROPEDGE_SHARED_LAYERS = 1, 2
TAP_PAIRED = 19                             # pair head: the rows the head reads, [n_pairs][D_last] (last layer)
TAP_HEAD_HIDDEN = 20                        # hidden head layer: Z1 of the last forward, [head_rows][Dh] (last layer)
READOUT_NONE, READOUT_MEAN, READOUT_SUM, READOUT_MAX = 0, 1, 2, 3      # graph-level readout (set_readout)
PAIR_NONE, PAIR_MUL, PAIR_ADD = 0, 1, 2                                # pair head (set_pairs)
PAIR_MODES = {"none": PAIR_NONE, "mul": PAIR_MUL, "add": PAIR_ADD}
NEG_NONE, NEG_UNIFORM, NEG_CORRUPT = 0, 1, 2                           # negative sampling (set_negative_sampling)
NEG_MODES = {"none": NEG_NONE, "uniform": NEG_UNIFORM, "corrupt": NEG_CORRUPT}
NEG_BOTH_DIRECTIONS, NEG_ALLOW_SELF = 1, 2
NEG_TRIES = 16
READOUT_MODES = {"none": READOUT_NONE, "mean": READOUT_MEAN, "sum": READOUT_SUM, "max": READOUT_MAX}
LOSS_SOFTMAX_CE, LOSS_BCE, LOSS_MSE = 0, 1, 2                          # loss modes of the output head (set_loss)
LOSS_MODES = {"softmax": LOSS_SOFTMAX_CE, "bce": LOSS_BCE, "mse": LOSS_MSE}
(K_PROJECT, K_EDGE_FWD, K_HEAD_FWD, K_HEAD_BWD, K_EDGE_BWD, K_GPL_SUM, K_GRAD_W, K_GRAD_X, K_MISC,
 K_EXCHANGE, K_EDGE_FUSED, K_COUNT) = range(12)
COMM_ID_BYTES = 128
PATH_GENERIC_SHAPE, PATH_FAST, PATH_GENERIC_SIZE = 0, 1, 2
GRAPH_SELF_LOOPS, GRAPH_SYMMETRIZE, GRAPH_COALESCE = 1, 2, 4      # flags of the graph builder (graph_from_coo, set_graph_coo)
CSR_OK, CSR_BAD_START, CSR_BAD_END, CSR_NOT_MONOTONE, CSR_COL_RANGE = range(5)   # graph_check_device

OPT_SGD, OPT_ADAM, OPT_ADAMW = 1, 2, 3                                 # optimizer on the device (set_optimizer)
OPT_KINDS = {"sgd": OPT_SGD, "adam": OPT_ADAM, "adamw": OPT_ADAMW}
OPT_NESTEROV = 1
CLIP_NONE, CLIP_PER_GROUP, CLIP_GLOBAL = 0, 1, 2
CLIP_MODES = {"none": CLIP_NONE, "group": CLIP_PER_GROUP, "global": CLIP_GLOBAL}
OPT_STATE_M, OPT_STATE_V, OPT_STATE_MOMENTUM = 0, 1, 2
DECAY_ALL_GROUPS = 0xFFFFFFFF

_lib: Optional[C.CDLL] = None


def build_library(force: bool = False) -> str:
    """Compile libgatv2_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def load_library(preload_torch: bool = True) -> C.CDLL:
    """dlopen the C-ABI library.  When torch is importable it is imported first so that this
    library binds to the HIP runtime torch already loaded (same soname), which is what lets
    torch.distributed/RCCL operate on the context's buffers and stream."""
    global _lib
    if _lib is not None:
        return _lib
    # GATV2_LIB: another build of the same ABI — the experiment library (csrc `make experiments`, libgatv2_hip_exp.so: the
    # timing-only GAT_DBG variants live only there) for tools/bench_ab.sh and the experiment-kernel tests
    lib_path = os.environ.get("GATV2_LIB") or LIB_PATH
    if not os.path.exists(lib_path):
        raise GatLibraryError(
            f"{lib_path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the HIP path)")
    if preload_torch:
        try:
            import torch  # noqa: F401
        except Exception:  # torch absent: fall back to the system HIP runtime
            pass
    try:
        lib = C.CDLL(lib_path, mode=C.RTLD_LOCAL)
    except OSError as e:
        raise GatLibraryError(f"cannot load {lib_path}: {e}") from e
    _declare(lib)
    _lib = lib
    return lib


def switches() -> str:
    """The choice switches (environment) this process has read and found set: "NAME=VALUE ..." (gat_switches)."""
    buf = C.create_string_buffer(4096)
    _chk(load_library().gat_switches(buf, 4096))
    return buf.value.decode()


def _declare(lib: C.CDLL) -> None:
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    P = C.POINTER
    lib.gat_last_error.restype = C.c_char_p
    lib.gat_last_error.argtypes = []
    lib.gat_kernel_name.restype = C.c_char_p
    lib.gat_kernel_name.argtypes = [C.c_int]
    sigs = {
        "gat_abi_version": [],
        "gat_device_count": [P(C.c_int)],
        "gat_switches": [C.c_char_p, i64],
        "gat_create": [P(_Config), P(vp)],
        "gat_destroy": [vp],
        "gat_sync": [vp],
        "gat_mem_info": [P(C.c_size_t), P(C.c_size_t)],
        "gat_set_graph": [vp, vp, vp, i64, i64, i64, i64],
        "gat_set_features": [vp, vp, i64, i32],
        "gat_set_labels": [vp, vp, i64],
        "gat_set_train_mask": [vp, vp, i64],
        "gat_eval_mask": [vp, vp, i64, P(C.c_double), P(i32), P(i32)],
        "gat_set_graph_device": [vp, vp, vp, i64, i64, i64, i64],
        "gat_set_features_device": [vp, vp, i64, i32],
        "gat_set_labels_device": [vp, vp, i64],
        "gat_set_source_features": [vp, vp, i64, i32],
        "gat_set_source_features_device": [vp, vp, i64, i32],
        "gat_param_count": [vp, C.c_int, P(i64)],
        "gat_params_init": [vp, C.c_uint64],
        "gat_params_set": [vp, C.c_int, vp, i64],
        "gat_params_get": [vp, C.c_int, vp, i64],
        "gat_grads_get": [vp, C.c_int, vp, i64],
        "gat_grads_set": [vp, C.c_int, vp, i64],
        "gat_grads_device": [vp, P(vp), P(i64)],
        "gat_grads_export": [vp, vp, i64],
        "gat_grads_import": [vp, vp, i64],
        "gat_result_export": [vp, vp],
        "gat_comm_unique_id": [vp],
        "gat_comm_init_rccl": [vp, i32, i32, vp],
        "gat_comm_init_host": [vp, i32, i32, C.c_char_p, i64],
        "gat_comm_option": [vp, i32, i32],
        "gat_comm_halo_info": [vp, P(i32), P(i64), P(i64), P(C.c_double)],
        "gat_step": [vp, P(f32), P(i32)],
        "gat_step_graph": [vp, i32],
        "gat_step_graph_state": [vp, P(i32)],
        "gat_forward": [vp, P(f32), P(i32)],
        "gat_backward": [vp],
        "gat_zero_grad": [vp],
        "gat_clip": [vp, f32],
        "gat_step_sgd": [vp, f32],
        "gat_step_adam": [vp, f32, f32, f32, f32, i32],
        "gat_set_optimizer": [vp, P(_OptimizerConfig)],
        "gat_optimizer_step": [vp],
        "gat_set_lr": [vp, f32],
        "gat_optimizer_info": [vp, P(_OptimizerConfig), P(i64), P(f32), P(f32), vp],
        "gat_optimizer_state_get": [vp, C.c_int, C.c_int, vp, i64],
        "gat_optimizer_state_set": [vp, C.c_int, C.c_int, vp, i64],
        "gat_optimizer_step_count_set": [vp, i64],
        "gat_train_step": [vp, P(f32), P(i32)],
        "gat_layer_project": [vp, i32],
        "gat_layer_forward_edges": [vp, i32],
        "gat_head_forward": [vp, P(f32), P(i32)],
        "gat_head_backward": [vp],
        "gat_layer_backward_edges": [vp, i32],
        "gat_layer_backward_dense": [vp, i32],
        "gat_layer_exchange": [vp, i32, P(i32)],
        "gat_layer_path": [vp, i32, P(i32)],
        "gat_table": [vp, C.c_int, i32, P(vp), P(i64), P(i64)],
        "gat_bind_table": [vp, C.c_int, i32, vp, i64],
        "gat_tap": [vp, C.c_int, i32, vp, i64],
        "gat_op_csr_to_coo": [vp, vp, vp, vp, i64, i64, vp],
        "gat_op_layer_forward": [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, i32, f32, vp],
        "gat_op_layer_backward": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, f32, vp],
        "gat_op_edge_score": [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i64, f32, vp],
        "gat_op_max_sum": [vp, vp, i64, i32, i64, vp, vp, vp],
        "gat_op_attn_coeff": [vp, vp, vp, vp, vp, vp, i64, i32, i64, vp],
        "gat_op_aggregate": [vp, vp, vp, vp, vp, vp, i64, i32, i64, i32, i32, vp],
        "gat_op_post_activation": [vp, vp, i64, i32, i32, i32, f32, vp],
        "gat_op_output_head": [vp, vp, vp, vp, i64, i32, i32, vp],
        "gat_op_loss_accuracy": [vp, vp, vp, vp, i64, i32, vp],
        "gat_op_output_gradients": [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, f32, i32, vp],
        "gat_op_grad_attn_coeff": [i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp],
        "gat_op_grad_attn_score": [vp, vp, vp, vp, vp, i64, i32, i64, vp],
        "gat_op_grad_parameters": [i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, i64, vp],
        "gat_op_features_input_gradients": [i64, i32, i64, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "gat_op_preact_gradient": [i64, f32, i32, vp, vp, vp],
        "gat_kernel_stats": [vp, C.c_int, P(i64), P(C.c_double)],
        "gat_kernel_stats_reset": [vp],
        "gat_algorithmic_bytes": [vp, P(C.c_double), P(C.c_double)],
        "gat_algorithmic_bytes_shape": [P(_Config), i64, i64, i64, i32, P(C.c_double), P(C.c_double)],
        "gat_request_bytes_shape": [P(_Config), i64, i64, i64, i32, P(C.c_double), P(C.c_double)],
        "gat_synth_sources_device": [vp, vp, vp, i64, i64, C.c_uint64, vp, vp],
        "gat_synth_features_device": [C.c_uint64, i64, i64, i32, i32, vp, vp],
        "gat_synth_labels_device": [C.c_uint64, i64, i64, i32, vp, vp],
        "gat_synth_argsort_u64": [vp, i64, vp, vp],
        "gat_set_dropout": [vp, f32, f32, C.c_uint64, C.c_uint64],
        "gat_set_dropedge": [vp, f32, i32],
        "gat_set_residual": [vp, i32],
        "gat_set_norm": [vp, i32, f32],
        "gat_set_batch_norm": [vp, i32, f32, f32],
        "gat_batch_norm_info": [vp, P(i32), P(f32), P(f32)],
        "gat_batch_norm_stats_get": [vp, i32, vp, i64],
        "gat_batch_norm_stats_set": [vp, i32, vp, i64],
        "gat_op_batch_norm_forward": [vp, i64, i32, i32, i32, vp, vp, f32, f32, f32, vp, vp, i32, vp, vp, vp],
        "gat_op_batch_norm_backward": [vp, vp, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, f32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "gat_set_edge_dim": [vp, i32],
        "gat_set_edge_features": [vp, vp, i64, i32],
        "gat_set_edge_features_device": [vp, vp, i64, i32],
        "gat_set_readout": [vp, i32, vp, i64],
        "gat_set_readout_device": [vp, i32, vp, i64],
        "gat_readout_info": [vp, P(i32), P(i64)],
        "gat_set_pairs": [vp, i32, vp, vp, i64],
        "gat_set_pairs_device": [vp, i32, vp, vp, i64],
        "gat_pairs_info": [vp, P(i32), P(i64)],
        "gat_op_pair_forward": [vp, i64, vp, vp, i64, i64, i32, i32, vp, vp],
        "gat_op_pair_backward": [vp, vp, i64, vp, vp, i64, i64, i32, i32, vp, i64, vp],
        "gat_set_head_hidden": [vp, i32, i32],
        "gat_head_hidden_info": [vp, P(i32), P(i32)],
        "gat_op_head_hidden_forward": [vp, vp, i64, i32, f32, vp],
        "gat_op_head_hidden_backward": [vp, vp, i64, i32, f32, vp, vp],
        "gat_set_negative_sampling": [vp, i32, i64, i64, i32, C.c_uint64],
        "gat_resample_negatives": [vp, C.c_uint64],
        "gat_negatives_info": [vp, P(i32), P(i64), P(i64), P(C.c_uint64), P(i64)],
        "gat_pairs_get": [vp, vp, vp, i64],
        "gat_op_negative_sample": [vp, vp, i64, i64, i32, i32, C.c_uint64, C.c_uint64, vp, vp, i64, vp, vp, i64, P(i64), vp],
        "gat_set_loss": [vp, i32],
        "gat_set_targets": [vp, vp, i64, i32],
        "gat_set_targets_device": [vp, vp, i64, i32],
        "gat_loss_info": [vp, P(i32), P(i32)],
        "gat_target_count": [vp, vp, i64, P(i64)],
        "gat_eval_rank": [vp, vp, i64, vp, i32, vp],
        "gat_op_rank_stats": [vp, i64, vp, vp, vp, i64, i32, vp, i32, vp, vp],
        "gat_op_readout_forward": [vp, i64, vp, i64, i64, i32, i32, vp, vp, vp],
        "gat_op_readout_backward": [vp, vp, i64, i64, i32, i32, vp, vp, i64, vp],
        "gat_op_dense_scratch_floats": [i32, i64, i32, i32, i32, P(i64)],
        "gat_op_dense_project": [vp, i32, vp, i64, i32, i32, i32, i32, vp, vp, vp, i64, vp, C.c_char_p, i32],
        "gat_op_dense_grad_x": [vp, vp, vp, vp, vp, i64, i32, i32, f32, vp, C.c_char_p, i32],
        "gat_op_dense_grad_w": [vp, vp, vp, i32, vp, vp, i64, i64, i32, i32, i32, vp, C.c_char_p, i32],
        "gat_op_dense_project_res": [vp, i32, vp, vp, i64, i32, i32, vp, C.c_char_p, i32],
        "gat_op_dense_grad_wres": [vp, vp, i32, vp, vp, i64, i64, i32, i32, vp, C.c_char_p, i32],
        "gat_op_dense_grad_x_res": [vp, vp, vp, i64, i32, i32, vp, C.c_char_p, i32],
        "gat_set_training": [vp, i32],
        "gat_dropout_step": [vp, P(C.c_uint64)],
        "gat_set_shard_bounds": [vp, i32, vp],
        "gat_graph_from_coo_device": [vp, vp, i64, i64, i64, i64, i32, vp, vp, i64, P(i64), vp],
        "gat_graph_from_coo": [vp, vp, i64, i64, i64, i64, i32, vp, vp, i64, P(i64), i32],
        "gat_set_graph_coo": [vp, vp, vp, i64, i64, i64, i64, i32],
        "gat_set_graph_coo_device": [vp, vp, vp, i64, i64, i64, i64, i32],
        "gat_graph_size": [vp, P(i64), P(i64), P(i64)],
        "gat_graph_get": [vp, vp, vp],
        "gat_graph_check_device": [vp, vp, i64, i64, i64, P(i32), P(i64), vp],
    }
    for name, argt in sigs.items():
        fn = getattr(lib, name)          # AttributeError here == symbol missing from the .so
        fn.argtypes = argt
        fn.restype = C.c_int


EXPORTED_SYMBOLS = None  # filled lazily by declared_symbols()


def declared_symbols() -> List[str]:
    """Function names declared in include/gatv2_abi.h (parsed from the header text)."""
    import re
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gat_[a-z0-9_]+)\s*\(", txt)))


def _chk(rc: int) -> None:
    if rc != 0:
        raise GatError(rc, load_library().gat_last_error().decode("utf-8", "replace"))


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class GatContext:
    """One GPU's (one rank's) context: mirrors the reference's per-process state — graph,
    features, labels, parameters and every intermediate of the epoch loop (E:1151-1357)."""

    def __init__(self, heads: Sequence[int], outdims: Sequence[int], in_dim: int, num_classes: int, *,
                 device: int = 0, stream: int = 0, negative_slope: float = 0.01,
                 flat_lrelu_index: bool = False, collect_timing: bool = False, keep_taps: bool = False,
                 dtype: str = "f32"):
        if len(heads) != len(outdims) or len(heads) == 0:
            raise ValueError("--heads and --outdims must both have num_layers values")
        self.lib = load_library()
        self.heads, self.outdims = list(map(int, heads)), list(map(int, outdims))
        self.L, self.in_dim, self.C = len(self.heads), int(in_dim), int(num_classes)
        self._h = (C.c_int32 * self.L)(*self.heads)
        self._d = (C.c_int32 * self.L)(*self.outdims)
        cfg = _Config(self.L, self._h, self._d, self.in_dim, self.C, negative_slope, device,
                      C.c_void_p(stream or None), int(flat_lrelu_index), int(collect_timing), int(keep_taps),
                      {"f32": 0, "bf16": 1}[dtype])
        self.storage_bytes = 2 if dtype == "bf16" else 4        # element size of the PL exchange table
        self._ctx = C.c_void_p()
        _chk(self.lib.gat_create(C.byref(cfg), C.byref(self._ctx)))
        self.n_rows = self.n_edges = self.n_table = 0
        self.table_row0 = 0
        self.n_graphs = 0                               # > 0 on a readout context (set_readout)
        self.n_pairs = 0                                # > 0 on a context with a pair head (set_pairs)
        self.head_hidden = 0                            # > 0 on a context with a hidden head layer (set_head_hidden)

    # -- lifecycle
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self.lib.gat_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        _chk(self.lib.gat_sync(self._ctx))

    # -- shapes
    @property
    def head_rows(self) -> int:
        """Rows of the output head — of labels, targets, masks and the y tap: the pairs of a pair head, the graphs of a readout
        context, else the nodes."""
        return self.n_pairs or self.n_graphs or self.n_rows

    @property
    def in_dims(self) -> List[int]:
        d = [self.in_dim]
        for l in range(1, self.L):
            d.append(self.heads[l - 1] * self.outdims[l - 1])
        return d

    def param_count(self, group: int) -> int:
        n = C.c_int64()
        _chk(self.lib.gat_param_count(self._ctx, group, C.byref(n)))
        return n.value

    # -- data
    def set_graph(self, row_ptr, col_idx, n_table: Optional[int] = None, table_row0: int = 0):
        rp = np.ascontiguousarray(row_ptr, np.int32)
        ci = np.ascontiguousarray(col_idx, np.int32)
        n, e = len(rp) - 1, len(ci)
        nt = n if n_table is None else int(n_table)
        _chk(self.lib.gat_set_graph(self._ctx, _np_ptr(rp), _np_ptr(ci), n, e, nt, table_row0))
        self.n_rows, self.n_edges, self.n_table, self.table_row0 = n, e, nt, table_row0

    def set_graph_device(self, d_row_ptr: int, d_col_idx: int, n_rows: int, n_edges: int,
                         n_table: Optional[int] = None, table_row0: int = 0):
        nt = n_rows if n_table is None else int(n_table)
        _chk(self.lib.gat_set_graph_device(self._ctx, C.c_void_p(d_row_ptr), C.c_void_p(d_col_idx), n_rows,
                                           n_edges, nt, table_row0))
        self.n_rows, self.n_edges, self.n_table, self.table_row0 = n_rows, n_edges, nt, table_row0

    def set_graph_coo(self, src, dst, n_rows: int, n_table: Optional[int] = None, table_row0: int = 0, flags: int = 0):
        """Build the CSR from the edge list (host arrays) on the device and train on it; see graph_from_coo."""
        s, d, nt = _coo_args(src, dst, n_rows, n_table, flags)
        _chk(self.lib.gat_set_graph_coo(self._ctx, _np_ptr(s), _np_ptr(d), len(s), n_rows, nt, table_row0, flags))
        self.n_rows, self.n_edges, self.n_table = self.graph_size()
        self.table_row0 = table_row0

    def set_graph_coo_device(self, d_src: int, d_dst: int, n_in: int, n_rows: int, n_table: Optional[int] = None,
                             table_row0: int = 0, flags: int = 0):
        nt = _coo_sizes(n_in, n_rows, n_table, flags)
        _chk(self.lib.gat_set_graph_coo_device(self._ctx, C.c_void_p(d_src), C.c_void_p(d_dst), n_in, n_rows, nt, table_row0, flags))
        self.n_rows, self.n_edges, self.n_table = self.graph_size()
        self.table_row0 = table_row0

    def graph_size(self):
        """(n_rows, n_edges, n_table) of the CSR the context trains on."""
        n, e, t = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self.lib.gat_graph_size(self._ctx, C.byref(n), C.byref(e), C.byref(t)))
        return n.value, e.value, t.value

    def graph(self):
        """(row_ptr, col_idx) of the CSR the context trains on, as host int32 arrays."""
        n, e, _ = self.graph_size()
        rp, ci = np.empty(n + 1, np.int32), np.empty(e, np.int32)
        _chk(self.lib.gat_graph_get(self._ctx, _np_ptr(rp), _np_ptr(ci)))
        return rp, ci

    def set_features(self, x):
        x = np.ascontiguousarray(x, np.float32)
        _chk(self.lib.gat_set_features(self._ctx, _np_ptr(x), x.shape[0], x.shape[1]))

    def set_features_device(self, d_x: int, n_rows: int, in_dim: int):
        _chk(self.lib.gat_set_features_device(self._ctx, C.c_void_p(d_x), n_rows, in_dim))

    def set_source_features(self, x_table):
        """Replicated layer-0 input: features of every source-table row, [n_table][F0] (instead of
        set_features; layer 0 then needs no exchange)."""
        x = np.ascontiguousarray(x_table, np.float32)
        _chk(self.lib.gat_set_source_features(self._ctx, _np_ptr(x), x.shape[0], x.shape[1]))

    def set_source_features_device(self, d_x: int, n_table: int, in_dim: int):
        _chk(self.lib.gat_set_source_features_device(self._ctx, C.c_void_p(d_x), n_table, in_dim))

    def set_labels(self, labels):
        lab = np.ascontiguousarray(labels, np.int32)
        _chk(self.lib.gat_set_labels(self._ctx, _np_ptr(lab), len(lab)))

    def set_train_mask(self, mask):
        """mask: bool/uint8 [head_rows] — nodes, graphs of a readout context or pairs of a pair head (None: every row trains, the
        reference's behaviour)."""
        if mask is None:
            _chk(self.lib.gat_set_train_mask(self._ctx, None, 0))
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        _chk(self.lib.gat_set_train_mask(self._ctx, _np_ptr(m), len(m)))

    def eval_mask(self, mask):
        """-> (loss sum, #correct, #rows) of the last forward over the head rows of `mask`: nodes, the graphs of a readout context or
        the pairs of a pair head."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        l, c, n = C.c_double(), C.c_int32(), C.c_int32()
        _chk(self.lib.gat_eval_mask(self._ctx, _np_ptr(m), len(m), C.byref(l), C.byref(c), C.byref(n)))
        return l.value, c.value, n.value

    def eval_rank(self, mask, ks=()):
        """Ranking metrics of the last forward over the head rows of `mask` (gat_eval_rank): a dict of arrays with one entry per output
        column — n_pos, n_neg, n_nan, auc_num, ap, mrr, hits [C][len(ks)] — plus the derived auc (NaN where n_pos * n_neg == 0) and
        hits_at (hits / n_pos; 1.0 where the column has fewer than K negatives, NaN where it has no positive)."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        k = np.ascontiguousarray(ks, np.int32).reshape(-1)
        out = np.zeros(self.C, RANK_STATS_DTYPE)
        _chk(self.lib.gat_eval_rank(self._ctx, _np_ptr(m), len(m), _np_ptr(k) if len(k) else None, len(k), _np_ptr(out)))
        return rank_stats_dict(out, len(k))

    def set_labels_device(self, d_labels: int, n_rows: int):
        _chk(self.lib.gat_set_labels_device(self._ctx, C.c_void_p(d_labels), n_rows))

    # -- parameters
    def params_init(self, seed: int):
        _chk(self.lib.gat_params_init(self._ctx, seed))

    def params_set(self, group: int, arr):
        a = np.ascontiguousarray(arr, np.float32).reshape(-1)
        _chk(self.lib.gat_params_set(self._ctx, group, _np_ptr(a), a.size))

    def params_get(self, group: int) -> np.ndarray:
        a = np.empty(self.param_count(group), np.float32)
        _chk(self.lib.gat_params_get(self._ctx, group, _np_ptr(a), a.size))
        return a

    def grads_get(self, group: int) -> np.ndarray:
        a = np.empty(self.param_count(group), np.float32)
        _chk(self.lib.gat_grads_get(self._ctx, group, _np_ptr(a), a.size))
        return a

    def grads_set(self, group: int, arr):
        """Overwrite one group of the gradient buffer (clip / optimizer without a model run)."""
        a = np.ascontiguousarray(arr, np.float32).reshape(-1)
        _chk(self.lib.gat_grads_set(self._ctx, group, _np_ptr(a), a.size))

    def grads_device(self):
        p, n = C.c_void_p(), C.c_int64()
        _chk(self.lib.gat_grads_device(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def grads_export(self, d_dst: int, count: int):
        _chk(self.lib.gat_grads_export(self._ctx, C.c_void_p(d_dst), count))

    def result_export(self, d_dst3: int):
        _chk(self.lib.gat_result_export(self._ctx, C.c_void_p(d_dst3)))

    def grads_import(self, d_src: int, count: int):
        _chk(self.lib.gat_grads_import(self._ctx, C.c_void_p(d_src), count))

    @property
    def n_params(self) -> int:
        return sum(self.param_count(g) for g in PARAM_GROUPS_ALL)

    # -- residual / bias (gatv2_abi.h "residual")
    def set_residual(self, linear: bool = False, bias: bool = False, flags: int = 0):
        """h_pre += Wres x' (linear) + b (bias) in every layer, with the parameter groups PARAM_WRES / PARAM_B.  Only before the
        first params_* / grads_* / set_graph* call on the context.  ``flags``: extra raw GAT_RES_* bits (or-ed in)."""
        _chk(self.lib.gat_set_residual(self._ctx, int(flags) | (RES_LINEAR if linear else 0) | (RES_BIAS if bias else 0)))

    # -- layer normalisation (gatv2_abi.h "layer normalisation")
    def set_norm(self, layer: bool = True, skip_last: bool = False, eps: float = 1e-5, flags: int = 0):
        """LayerNorm over each row's H*D channels between the aggregation and the LeakyReLU, in every layer (``skip_last``: every layer
        but the last), with the parameter groups PARAM_LN_G / PARAM_LN_B.  Only before the first params_* / grads_* / set_graph*
        call on the context.  ``flags``: extra raw GAT_NORM_* bits (or-ed in)."""
        _chk(self.lib.gat_set_norm(self._ctx, int(flags) | (NORM_LAYER if layer else 0) | (NORM_SKIP_LAST if skip_last else 0), float(eps)))

    # -- batch normalisation (gatv2_abi.h "batch normalisation")
    def set_batch_norm(self, skip_last: bool = False, eps: float = 1e-5, momentum: float = 0.1, flags: int = BN_ON):
        """BatchNorm over the columns of each layer's [n_rows][H*D] aggregate between the aggregation and the LeakyReLU, in every layer
        (``skip_last``: every layer but the last), with gamma / beta in PARAM_NORM_G / PARAM_NORM_B and running statistics that
        advance once per training forward and are what eval mode (set_training(False)) normalises with.  Only before the first
        params_* / grads_* / set_graph* call on the context.  ``flags``: the raw GAT_BN_* bits (0: the call changes nothing)."""
        _chk(self.lib.gat_set_batch_norm(self._ctx, int(flags) | (BN_SKIP_LAST if skip_last else 0), float(eps), float(momentum)))

    def batch_norm_info(self):
        """(flags, eps, momentum) of the context's batch normalisation; flags 0 = off."""
        f, e, m = C.c_int32(0), C.c_float(0), C.c_float(0)
        _chk(self.lib.gat_batch_norm_info(self._ctx, C.byref(f), C.byref(e), C.byref(m)))
        return f.value, e.value, m.value

    def _bn_count(self) -> int:
        return sum(h * d for h, d in zip(self.heads, self.outdims))

    def batch_norm_stats(self, which: int) -> np.ndarray:
        """One of the BN_* statistics vectors, flat [l][H_l*D_l] over all layers."""
        out = np.empty(self._bn_count(), np.float32)
        _chk(self.lib.gat_batch_norm_stats_get(self._ctx, int(which), _np_ptr(out), out.size))
        return out

    def set_batch_norm_stats(self, which: int, arr):
        """Replaces BN_RUNNING_MEAN or BN_RUNNING_VAR (flat [l][H_l*D_l]); a captured step graph stays valid."""
        a = np.ascontiguousarray(arr, np.float32).ravel()
        _chk(self.lib.gat_batch_norm_stats_set(self._ctx, int(which), _np_ptr(a), a.size))

    # -- edge features (gatv2_abi.h "edge features")
    def set_edge_dim(self, edge_dim: int):
        """Per-edge attributes of ``edge_dim`` floats enter the attention score through the parameter group PARAM_WE (PyG's
        GATv2Conv ``edge_dim``).  Only before the first params_* / grads_* / set_graph* call on the context; 0 = off."""
        _chk(self.lib.gat_set_edge_dim(self._ctx, int(edge_dim)))

    def set_edge_features(self, ea):
        """The attribute rows [n_edges][edge_dim] in the order of the context's CSR (what graph() returns); after set_graph*."""
        a = np.ascontiguousarray(ea, np.float32)
        if a.ndim != 2:
            raise ValueError(f"edge features must be [n_edges][edge_dim], got shape {a.shape}")
        _chk(self.lib.gat_set_edge_features(self._ctx, _np_ptr(a), a.shape[0], a.shape[1]))

    def set_edge_features_device(self, d_ea: int, n_edges: int, edge_dim: int):
        _chk(self.lib.gat_set_edge_features_device(self._ctx, C.c_void_p(d_ea or None), n_edges, edge_dim))

    # -- hidden layer in front of the output head (gatv2_abi.h "hidden layer")
    def set_head_hidden(self, width: int, act="relu"):
        """One hidden layer of ``width`` units in front of the output head, for every head kind: Z1 = act(Xin W1^T + b1) with the
        parameter groups PARAM_HEAD_W [width][D_last] / PARAM_HEAD_B [width]; PARAM_WO becomes [C][width].  act: "relu", "lrelu" (the
        context's negative_slope) or the raw GAT_HEAD_ACT_* flags.  Only before the first params_* / grads_* / set_graph* call; 0 = off."""
        _chk(self.lib.gat_set_head_hidden(self._ctx, int(width), head_act(act)))
        self.head_hidden = int(width)

    def head_hidden_info(self):
        """(width, flags); (0, 0) while off."""
        w, f = C.c_int32(), C.c_int32()
        _chk(self.lib.gat_head_hidden_info(self._ctx, C.byref(w), C.byref(f)))
        return w.value, f.value

    # -- graph-level readout (gatv2_abi.h "graph-level readout")
    def set_readout(self, mode, graph_ptr=None, batch=None):
        """One label per GRAPH: the last layer's rows are pooled per graph ("mean", "sum", "max" or the GAT_READOUT_* integer) in front
        of the output head.  graph_ptr [n_graphs + 1]: graph g owns rows graph_ptr[g] .. graph_ptr[g+1]-1 (PyG's Batch.ptr); or batch
        [n_rows]: the sorted graph id of every row (PyG's Batch.batch; an unsorted one raises ValueError).  After set_graph*, before
        set_labels; labels and masks are then per graph.  Mode 0 / "none" leaves the context as it is."""
        m = readout_mode(mode)
        if m == READOUT_NONE:
            _chk(self.lib.gat_set_readout(self._ctx, m, None, 0))
            return
        if (graph_ptr is None) == (batch is None):
            raise ValueError("set_readout: give graph_ptr or batch (one of them)")
        gp = batch_to_graph_ptr(batch) if graph_ptr is None else np.ascontiguousarray(graph_ptr, np.int32)
        if gp.ndim != 1 or len(gp) < 2:
            raise ValueError("graph_ptr must be one-dimensional with n_graphs + 1 >= 2 entries")
        _chk(self.lib.gat_set_readout(self._ctx, m, _np_ptr(gp), len(gp) - 1))
        self.n_graphs = len(gp) - 1

    def set_readout_device(self, mode, d_graph_ptr: int, n_graphs: int):
        """set_readout on a device graph_ptr [n_graphs + 1] (checked on the device)."""
        _chk(self.lib.gat_set_readout_device(self._ctx, readout_mode(mode), C.c_void_p(d_graph_ptr or None), n_graphs))
        self.n_graphs = int(n_graphs)

    def readout_info(self):
        """(mode, n_graphs); (0, 0) while readout is off."""
        m, g = C.c_int32(), C.c_int64()
        _chk(self.lib.gat_readout_info(self._ctx, C.byref(m), C.byref(g)))
        return m.value, g.value

    # -- pair head (gatv2_abi.h "pair head")
    def set_pairs(self, mode, u=None, v=None):
        """One label per PAIR of nodes: the head reads Q[p] = X[u_p] * X[v_p] ("mul") or X[u_p] + X[v_p] ("add", or the GAT_PAIR_*
        integer) of the last layer's rows.  After set_graph*, before set_labels / set_targets; labels, targets and masks are then per
        pair.  A later call with the same mode and length replaces the pairs.  Mode 0 / "none" leaves the context as it is."""
        m = pair_mode(mode)
        if m == PAIR_NONE:
            _chk(self.lib.gat_set_pairs(self._ctx, m, None, None, 0))
            return
        if u is None or v is None:
            raise ValueError("set_pairs: give u and v")
        ua, va = np.ascontiguousarray(u, np.int32), np.ascontiguousarray(v, np.int32)
        if ua.ndim != 1 or ua.shape != va.shape:
            raise ValueError("u and v must be one-dimensional and of the same length")
        _chk(self.lib.gat_set_pairs(self._ctx, m, _np_ptr(ua), _np_ptr(va), len(ua)))
        self.n_pairs = len(ua)

    def set_pairs_device(self, mode, d_u: int, d_v: int, n_pairs: int):
        """set_pairs on device arrays [n_pairs] (checked on the device)."""
        m = pair_mode(mode)
        _chk(self.lib.gat_set_pairs_device(self._ctx, m, C.c_void_p(d_u or None), C.c_void_p(d_v or None), n_pairs))
        if m != PAIR_NONE:
            self.n_pairs = int(n_pairs)

    def pairs_info(self):
        """(mode, n_pairs); (0, 0) while the pair head is off."""
        m, n = C.c_int32(), C.c_int64()
        _chk(self.lib.gat_pairs_info(self._ctx, C.byref(m), C.byref(n)))
        return m.value, n.value

    def pairs(self):
        """The current pair lists (u [n_pairs] int32, v [n_pairs] int32), copied from the device: what a resample drew."""
        _, n = self.pairs_info()
        u, v = np.empty(n, np.int32), np.empty(n, np.int32)
        _chk(self.lib.gat_pairs_get(self._ctx, _np_ptr(u), _np_ptr(v), n))
        return u, v

    # -- negative sampling (gatv2_abi.h "negative sampling")
    def set_negative_sampling(self, mode, first=0, count=0, both_directions=False, allow_self=False, seed=0):
        """Pairs [first, first + count) of the pair list become the slots resample_negatives redraws: "uniform" node pairs or
        "corrupt" (one endpoint of source pair j % first, of pairs [0, first), replaced), never an edge of the context's graph — in
        either direction with both_directions — nor a self pair unless allow_self.  Labels, targets and masks over the slots stay the
        caller's.  Mode 0 / "none" switches it off.  Draws nothing itself."""
        flags = (NEG_BOTH_DIRECTIONS if both_directions else 0) | (NEG_ALLOW_SELF if allow_self else 0)
        _chk(self.lib.gat_set_negative_sampling(self._ctx, neg_mode(mode), int(first), int(count), flags, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def resample_negatives(self, round):
        """Draw round `round` into the negative slots (the law of synth.negative_pairs, bit for bit), rebuild the pair index and the
        work list on the device; a captured step_graph re-arms as after a replacing set_pairs."""
        _chk(self.lib.gat_resample_negatives(self._ctx, int(round) & 0xFFFFFFFFFFFFFFFF))

    def negatives_info(self):
        """(mode, first, count, last round drawn, its unfiltered count); zeros while off."""
        m, f, n, r, uf = C.c_int32(), C.c_int64(), C.c_int64(), C.c_uint64(), C.c_int64()
        _chk(self.lib.gat_negatives_info(self._ctx, C.byref(m), C.byref(f), C.byref(n), C.byref(r), C.byref(uf)))
        return m.value, f.value, n.value, r.value, uf.value

    # -- loss modes of the output head (gatv2_abi.h "loss modes of the output head")
    def set_loss(self, mode):
        """"softmax" (the default: int32 labels, set_labels), "bce" or "mse" (float targets [rows][C] with NaN = missing, set_targets),
        or the GAT_LOSS_* integer.  Only before the first set_labels / set_targets call."""
        _chk(self.lib.gat_set_loss(self._ctx, loss_mode(mode)))

    def set_targets(self, t):
        """Targets [head_rows][C] — nodes, graphs of a readout context or pairs of a pair head — as floats; NaN marks a missing entry.  After set_graph* (and
        set_readout).  A later call with the same shape replaces the values in place (a captured step reads the new ones)."""
        a = np.ascontiguousarray(t, np.float32)
        if a.ndim != 2:
            raise ValueError(f"targets must be [n_rows][n_cols], got shape {a.shape}")
        _chk(self.lib.gat_set_targets(self._ctx, _np_ptr(a), a.shape[0], a.shape[1]))

    def set_targets_device(self, d_t: int, n_rows: int, n_cols: int):
        """set_targets on a device array (checked on the device)."""
        _chk(self.lib.gat_set_targets_device(self._ctx, C.c_void_p(d_t or None), n_rows, n_cols))

    def loss_info(self):
        """(mode, n_cols); (0, num_classes) by default."""
        m, n = C.c_int32(), C.c_int32()
        _chk(self.lib.gat_loss_info(self._ctx, C.byref(m), C.byref(n)))
        return m.value, n.value

    def target_count(self, mask=None) -> int:
        """Present (non-NaN) target entries in the rows of `mask`; None: in the current training set.  The denominator of the loss sum."""
        n = C.c_int64()
        if mask is None:
            _chk(self.lib.gat_target_count(self._ctx, None, 0, C.byref(n)))
        else:
            m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
            _chk(self.lib.gat_target_count(self._ctx, _np_ptr(m), len(m), C.byref(n)))
        return n.value

    # -- dropout (gatv2_abi.h "dropout")
    def set_dropout(self, feat_p: float = 0.0, attn_p: float = 0.0, seed: int = 0, first_step: int = 0):
        """Inverted feature / attention dropout in training mode; p in [0, 1).  The mask counter starts at first_step."""
        _chk(self.lib.gat_set_dropout(self._ctx, float(feat_p), float(attn_p), int(seed) & (2 ** 64 - 1), int(first_step)))

    def set_dropedge(self, p: float = 0.0, keep_self: bool = False, shared_layers: bool = False, flags: int = 0):
        """DropEdge in training mode (gatv2_abi.h "DropEdge"): every step drops each edge with probability p in [0, 1) before
        the softmax.  keep_self: self-loops are never dropped; shared_layers: one mask per step for all layers.  Seed and
        counter are those of set_dropout.  ``flags``: extra raw GAT_DROPEDGE_* bits (or-ed in)."""
        f = int(flags) | (DROPEDGE_KEEP_SELF if keep_self else 0) | (DROPEDGE_SHARED_LAYERS if shared_layers else 0)
        _chk(self.lib.gat_set_dropedge(self._ctx, float(p), f))

    def set_training(self, training: bool = True):
        """False: eval mode (no dropout, the counter does not advance)."""
        _chk(self.lib.gat_set_training(self._ctx, int(bool(training))))

    def dropout_step(self) -> int:
        st = C.c_uint64()
        _chk(self.lib.gat_dropout_step(self._ctx, C.byref(st)))
        return st.value

    def set_shard_bounds(self, bounds):
        """Global row boundaries [world+1] of the shard plan: the masks use unsharded node ids."""
        b = np.ascontiguousarray(bounds, np.int64)
        _chk(self.lib.gat_set_shard_bounds(self._ctx, len(b) - 1, _np_ptr(b)))

    # -- step
    def forward(self, want_loss: bool = True):
        if not want_loss:
            _chk(self.lib.gat_forward(self._ctx, None, None))
            return None
        loss, corr = C.c_float(), C.c_int32()
        _chk(self.lib.gat_forward(self._ctx, C.byref(loss), C.byref(corr)))
        return loss.value, corr.value

    def backward(self):
        _chk(self.lib.gat_backward(self._ctx))

    def step(self, want_loss: bool = True):
        """forward + backward (with a transport attached: exchanges and the single all-reduce inside)."""
        if not want_loss:
            _chk(self.lib.gat_step(self._ctx, None, None))
            return None
        loss, corr = C.c_float(), C.c_int32()
        _chk(self.lib.gat_step(self._ctx, C.byref(loss), C.byref(corr)))
        return loss.value, corr.value

    def step_graph(self, enable: bool = True):
        """step() as one replayed hipGraph launch (small, launch-bound graphs)."""
        _chk(self.lib.gat_step_graph(self._ctx, int(enable)))

    def step_graph_state(self) -> int:
        """0 off, 1 armed (the next step runs eagerly or captures), 2 captured (the next step is a replay)."""
        s = C.c_int32()
        _chk(self.lib.gat_step_graph_state(self._ctx, C.byref(s)))
        return s.value

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _chk(load_library().gat_comm_unique_id(buf))
        return buf.raw

    def comm_init_rccl(self, world: int, rank: int, unique_id: bytes):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique id must be COMM_ID_BYTES long")
        _chk(self.lib.gat_comm_init_rccl(self._ctx, world, rank, C.c_char_p(unique_id)))

    def comm_init_host(self, world: int, rank: int, shm_name: str, bytes_per_rank: int):
        _chk(self.lib.gat_comm_init_host(self._ctx, world, rank, shm_name.encode(), bytes_per_rank))

    def comm_option(self, option: int, value: int):
        _chk(self.lib.gat_comm_option(self._ctx, option, value))

    def comm_halo_info(self):
        """(active, rows received, rows sent, referenced fraction) of GAT_COMM_HALO."""
        act, rr, rs, fr = C.c_int32(), C.c_int64(), C.c_int64(), C.c_double()
        _chk(self.lib.gat_comm_halo_info(self._ctx, C.byref(act), C.byref(rr), C.byref(rs), C.byref(fr)))
        return bool(act.value), rr.value, rs.value, fr.value

    def zero_grad(self):
        _chk(self.lib.gat_zero_grad(self._ctx))

    def clip(self, threshold: float = 5.0):
        _chk(self.lib.gat_clip(self._ctx, threshold))

    def step_sgd(self, lr: float):
        _chk(self.lib.gat_step_sgd(self._ctx, lr))

    def step_adam(self, lr: float, beta1: float, beta2: float, eps: float, t: int):
        _chk(self.lib.gat_step_adam(self._ctx, lr, beta1, beta2, eps, t))

    # -- optimizer on the device (gatv2_abi.h "optimizer")
    def set_optimizer(self, kind, lr: float, *, momentum: float = 0.0, nesterov: bool = False, betas=(0.9, 0.999), eps: float = 1e-8,
                      weight_decay: float = 0.0, decay_groups=None, clip=None, flags: int = 0):
        """Configure the optimizer whose step runs on the device: ``kind`` "sgd" | "adam" | "adamw" (or an OPT_* value); ``decay_groups``
        None = every group (torch's behaviour), a bit mask, or an iterable of PARAM_* groups that take the weight decay; ``clip`` None,
        ("group", thr) = every group by its own norm (clip()'s law) or ("global", thr) = clip_grad_norm_ over all parameters.  Counts
        as a first params_* call (the packed sizes are final) and drops a captured step graph.  ``flags``: raw OPT_* bits (or-ed in)."""
        q = _OptimizerConfig()
        q.kind = OPT_KINDS[kind] if isinstance(kind, str) else int(kind)
        q.flags = int(flags) | (OPT_NESTEROV if nesterov else 0)
        q.lr, q.momentum, q.beta1, q.beta2, q.eps, q.weight_decay = float(lr), float(momentum), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
        if decay_groups is None:
            q.decay_groups = DECAY_ALL_GROUPS
        elif isinstance(decay_groups, (int, np.integer)):
            q.decay_groups = int(decay_groups)
        else:
            q.decay_groups = sum(1 << int(g) for g in set(decay_groups))
        if clip is None:
            q.clip_mode, q.clip_threshold = CLIP_NONE, 0.0
        else:
            mode, thr = clip
            q.clip_mode = CLIP_MODES[mode] if isinstance(mode, str) else int(mode)
            q.clip_threshold = float(thr)
        _chk(self.lib.gat_set_optimizer(self._ctx, C.byref(q)))

    def optimizer_step(self):
        """Clip and update in two launches, from the packed gradients as they are (they are only read)."""
        _chk(self.lib.gat_optimizer_step(self._ctx))

    def set_lr(self, lr: float):
        """Write the device learning rate on the context's stream; a captured step graph stays valid."""
        _chk(self.lib.gat_set_lr(self._ctx, float(lr)))

    def optimizer_info(self) -> dict:
        """The configuration, the device step count ``t`` and ``lr``, and the norms of the last step: ``group_norms`` [10], ``global_norm``."""
        q, t, lr, gn = _OptimizerConfig(), C.c_int64(), C.c_float(), C.c_float()
        norms = np.zeros(len(PARAM_GROUPS_ALL), np.float32)
        _chk(self.lib.gat_optimizer_info(self._ctx, C.byref(q), C.byref(t), C.byref(lr), C.byref(gn), _np_ptr(norms)))
        out = {name: getattr(q, name) for name, _ in _OptimizerConfig._fields_}
        out.update(t=t.value, lr=lr.value, global_norm=gn.value, group_norms=norms)
        return out

    def optimizer_state(self, which: int, group: int) -> np.ndarray:
        """One group of an optimizer state buffer (OPT_STATE_M / _V / _MOMENTUM), flat like params_get."""
        a = np.empty(self.param_count(group), np.float32)
        _chk(self.lib.gat_optimizer_state_get(self._ctx, int(which), int(group), _np_ptr(a), a.size))
        return a

    def set_optimizer_state(self, which: int, group: int, arr):
        a = np.ascontiguousarray(arr, np.float32).reshape(-1)
        _chk(self.lib.gat_optimizer_state_set(self._ctx, int(which), int(group), _np_ptr(a), a.size))

    def set_optimizer_step_count(self, t: int):
        _chk(self.lib.gat_optimizer_step_count_set(self._ctx, int(t)))

    def train_step(self, want_loss: bool = True):
        """zero_grad + step + optimizer_step as one call (with step_graph(True): one replayed launch).  Returns (loss sum, #correct) of the
        forward before the update."""
        if not want_loss:
            _chk(self.lib.gat_train_step(self._ctx, None, None))
            return None
        loss, corr = C.c_float(), C.c_int32()
        _chk(self.lib.gat_train_step(self._ctx, C.byref(loss), C.byref(corr)))
        return loss.value, corr.value

    # -- phases
    def layer_project(self, l: int):
        _chk(self.lib.gat_layer_project(self._ctx, l))

    def layer_forward_edges(self, l: int):
        _chk(self.lib.gat_layer_forward_edges(self._ctx, l))

    def head_forward(self, want_loss: bool = True):
        if not want_loss:
            _chk(self.lib.gat_head_forward(self._ctx, None, None))
            return None
        loss, corr = C.c_float(), C.c_int32()
        _chk(self.lib.gat_head_forward(self._ctx, C.byref(loss), C.byref(corr)))
        return loss.value, corr.value

    def head_backward(self):
        _chk(self.lib.gat_head_backward(self._ctx))

    def layer_backward_edges(self, l: int):
        _chk(self.lib.gat_layer_backward_edges(self._ctx, l))

    def layer_backward_dense(self, l: int):
        _chk(self.lib.gat_layer_backward_dense(self._ctx, l))

    def layer_exchange(self, l: int) -> bool:
        need = C.c_int32(0)
        _chk(self.lib.gat_layer_exchange(self._ctx, l, C.byref(need)))
        return bool(need.value)

    def layer_path(self, l: int) -> int:
        """PATH_FAST / PATH_GENERIC_SHAPE / PATH_GENERIC_SIZE: the edge kernels layer l runs on."""
        p = C.c_int32(0)
        _chk(self.lib.gat_layer_path(self._ctx, l, C.byref(p)))
        return p.value

    def last_message(self) -> str:
        """gat_last_error(): after a successful call either stale text or a "warning: ..." left by that call."""
        return self.lib.gat_last_error().decode("utf-8", "replace")

    def table(self, which: int, l: int):
        p, n, w = C.c_void_p(), C.c_int64(), C.c_int64()
        _chk(self.lib.gat_table(self._ctx, which, l, C.byref(p), C.byref(n), C.byref(w)))
        return p.value, n.value, w.value

    def bind_table(self, which: int, l: int, d_ptr: int, nbytes: int):
        _chk(self.lib.gat_bind_table(self._ctx, which, l, C.c_void_p(d_ptr), nbytes))

    # -- taps (reference layouts)
    def tap(self, tensor: int, l: int = 0) -> np.ndarray:
        N, E = self.n_rows, self.n_edges
        H, D = self.heads[l], self.outdims[l]
        last = l == self.L - 1
        G = self.n_graphs                               # readout: the pooled rows
        shapes = {
            TAP_SRC: ((E,), np.int32), TAP_DST: ((E,), np.int32),
            TAP_ALPHA: ((H, E), np.float32), TAP_GE: ((H, E), np.float32),
            TAP_MAX: ((H, N), np.float32), TAP_SUM: ((H, N), np.float32),
            TAP_HPRE: ((N, H, D), np.float32), TAP_G: ((N, H, D), np.float32),
            TAP_HOUT: ((N, D if last else H * D), np.float32),
            TAP_Y: ((self.head_rows, self.C), np.float32),
            TAP_POOLED: ((G, self.outdims[-1]), np.float32),
            TAP_PAIRED: ((self.n_pairs, self.outdims[-1]), np.float32),
            TAP_HEAD_HIDDEN: ((self.head_rows, self.head_hidden), np.float32),
            TAP_PL: ((self.n_table, H * D), np.float32), TAP_PR: ((N, H * D), np.float32),
            TAP_SCORE: ((H, E), np.float32), TAP_GALPHA: ((H, E), np.float32),
            TAP_GX: ((N, self.heads[l - 1] * self.outdims[l - 1] if l > 0 else 0), np.float32),
            TAP_ATTN_KEEP: ((H, E), np.float32), TAP_FEAT_KEEP: ((N, self.in_dims[l]), np.float32),
            TAP_EDGE_KEEP: ((E,), np.float32),
        }
        shape, dt = shapes[tensor]
        out = np.empty(shape, dt)
        _chk(self.lib.gat_tap(self._ctx, tensor, l, _np_ptr(out), out.size))
        return out

    # -- measurement
    def kernel_stats(self):
        out = {}
        for k in range(K_COUNT):
            n, ms = C.c_int64(), C.c_double()
            _chk(self.lib.gat_kernel_stats(self._ctx, k, C.byref(n), C.byref(ms)))
            out[self.lib.gat_kernel_name(k).decode()] = (n.value, ms.value)
        return out

    def kernel_stats_reset(self):
        _chk(self.lib.gat_kernel_stats_reset(self._ctx))

    def algorithmic_bytes(self):
        tot = C.c_double()
        per = (C.c_double * K_COUNT)()
        _chk(self.lib.gat_algorithmic_bytes(self._ctx, C.byref(tot), per))
        return tot.value, {self.lib.gat_kernel_name(k).decode(): per[k] for k in range(K_COUNT)}


def algorithmic_bytes_shape(heads: Sequence[int], outdims: Sequence[int], in_dim: int, num_classes: int, n_rows: int,
                            n_edges: int, *, dtype: str = "f32", n_table: Optional[int] = None, replicated_input: bool = False):
    """SURVEY 8d's algorithmic HBM bytes of one forward+backward step from the shape alone (host arithmetic: works
    without a GPU).  -> (bytes_step, {kernel class: bytes})"""
    lib = load_library()
    L = len(heads)
    h = (C.c_int32 * L)(*heads); d = (C.c_int32 * L)(*outdims)
    cfg = _Config()
    cfg.num_layers, cfg.heads, cfg.outdims = L, h, d
    cfg.in_dim, cfg.num_classes = int(in_dim), int(num_classes)
    cfg.storage_dtype = 1 if dtype == "bf16" else 0
    tot = C.c_double()
    per = (C.c_double * K_COUNT)()
    _chk(lib.gat_algorithmic_bytes_shape(C.byref(cfg), n_rows, n_edges, n_rows if n_table is None else n_table,
                                         int(replicated_input), C.byref(tot), per))
    return tot.value, {lib.gat_kernel_name(k).decode(): per[k] for k in range(K_COUNT)}


def request_bytes_shape(heads: Sequence[int], outdims: Sequence[int], in_dim: int, num_classes: int, n_rows: int,
                        n_edges: int, *, dtype: str = "f32", n_table: Optional[int] = None, replicated_input: bool = False):
    """The same byte model with every per-edge gathered / scattered row rounded up to whole 128-byte fabric requests
    (gat_request_bytes_shape): the roofline the memory system can serve.  -> (bytes_step, {kernel class: bytes})"""
    lib = load_library()
    L = len(heads)
    h = (C.c_int32 * L)(*heads); d = (C.c_int32 * L)(*outdims)
    cfg = _Config()
    cfg.num_layers, cfg.heads, cfg.outdims = L, h, d
    cfg.in_dim, cfg.num_classes = int(in_dim), int(num_classes)
    cfg.storage_dtype = 1 if dtype == "bf16" else 0
    tot = C.c_double()
    per = (C.c_double * K_COUNT)()
    _chk(lib.gat_request_bytes_shape(C.byref(cfg), n_rows, n_edges, n_rows if n_table is None else n_table,
                                     int(replicated_input), C.byref(tot), per))
    return tot.value, {lib.gat_kernel_name(k).decode(): per[k] for k in range(K_COUNT)}


def readout_mode(mode) -> int:
    """"mean" / "sum" / "max" / "none" or the GAT_READOUT_* integer -> the integer."""
    if isinstance(mode, str):
        if mode not in READOUT_MODES:
            raise ValueError(f"readout mode must be one of {sorted(READOUT_MODES)}, got {mode!r}")
        return READOUT_MODES[mode]
    return int(mode)


def pair_mode(mode) -> int:
    """"mul" / "add" / "none" or the GAT_PAIR_* integer -> the integer."""
    if isinstance(mode, str):
        if mode not in PAIR_MODES:
            raise ValueError(f"pair mode must be one of {sorted(PAIR_MODES)}, got {mode!r}")
        return PAIR_MODES[mode]
    return int(mode)


def neg_mode(mode) -> int:
    """"uniform" / "corrupt" / "none" or the GAT_NEG_* integer -> the integer."""
    if isinstance(mode, str):
        if mode not in NEG_MODES:
            raise ValueError(f"negative sampling mode must be one of {sorted(NEG_MODES)}, got {mode!r}")
        return NEG_MODES[mode]
    return int(mode)


def loss_mode(mode) -> int:
    """"softmax" / "bce" / "mse" or the GAT_LOSS_* integer -> the integer."""
    if isinstance(mode, str):
        if mode not in LOSS_MODES:
            raise ValueError(f"loss mode must be one of {sorted(LOSS_MODES)}, got {mode!r}")
        return LOSS_MODES[mode]
    return int(mode)


def head_act(act) -> int:
    """"relu" / "lrelu" or the GAT_HEAD_ACT_* flags -> the flags."""
    if isinstance(act, str):
        if act not in HEAD_ACTS:
            raise ValueError(f"head activation must be one of {sorted(HEAD_ACTS)}, got {act!r}")
        return HEAD_ACTS[act]
    return int(act)


def batch_to_graph_ptr(batch) -> np.ndarray:
    """A sorted graph id per row (PyG's Batch.batch) -> graph_ptr [n_graphs + 1] int32, n_graphs = batch[-1] + 1 (ids that do not
    occur are empty graphs).  ValueError for an unsorted, negative or empty vector."""
    b = np.asarray(batch)
    if b.ndim != 1 or b.size == 0:
        raise ValueError("batch must be a non-empty one-dimensional vector")
    if b.dtype.kind not in "iu":
        raise TypeError(f"batch must hold integers, got {b.dtype}")
    if int(b.min()) < 0:
        raise ValueError("batch holds a negative graph id")
    if np.any(np.diff(b.astype(np.int64)) < 0):
        raise ValueError("batch must be sorted (the rows of a graph are contiguous)")
    g = int(b[-1]) + 1
    return np.searchsorted(b, np.arange(g + 1)).astype(np.int32)


def op_readout_forward(d_x: int, x_stride: int, d_graph_ptr: int, n_graphs: int, n_rows: int, width: int, mode, d_pooled: int,
                       d_argmax: int = 0, stream: int = 0):
    """gat_op_readout_forward on device pointers: pooled [n_graphs][width] (and argmax for "max") of the rows of x."""
    _chk(load_library().gat_op_readout_forward(C.c_void_p(d_x or None), x_stride, C.c_void_p(d_graph_ptr or None), n_graphs, n_rows, width,
                                               readout_mode(mode), C.c_void_p(d_pooled or None), C.c_void_p(d_argmax or None),
                                               C.c_void_p(stream or None)))


def op_readout_backward(d_gpooled: int, d_graph_ptr: int, n_graphs: int, n_rows: int, width: int, mode, d_argmax: int, d_gh: int,
                        gh_stride: int, stream: int = 0):
    """gat_op_readout_backward on device pointers: floats 0..width-1 of every gh row from the pooled gradient."""
    _chk(load_library().gat_op_readout_backward(C.c_void_p(d_gpooled or None), C.c_void_p(d_graph_ptr or None), n_graphs, n_rows, width,
                                                readout_mode(mode), C.c_void_p(d_argmax or None), C.c_void_p(d_gh or None), gh_stride,
                                                C.c_void_p(stream or None)))


def op_batch_norm_forward(d_u: int, n_rows: int, H: int, D: int, is_last: bool, d_gamma: int, d_beta: int, eps: float, slope: float,
                          momentum: float, d_running_mean: int, d_running_var: int, training: bool, d_mean_rstd: int, d_hout: int,
                          stream: int = 0):
    """gat_op_batch_norm_forward on device pointers: hout of u [n_rows][H*D]; training: {mu, rstd} into d_mean_rstd [2][H*D] and the
    running pair (0: none) advanced; eval: the running pair is what is normalised with."""
    p = lambda x: C.c_void_p(x or None)
    _chk(load_library().gat_op_batch_norm_forward(p(d_u), n_rows, H, D, int(bool(is_last)), p(d_gamma), p(d_beta), eps, slope, momentum,
                                                  p(d_running_mean), p(d_running_var), int(bool(training)), p(d_mean_rstd), p(d_hout), p(stream)))


def op_batch_norm_backward(d_u: int, d_g: int, d_gh: int, gh_stride: int, n_rows: int, H: int, D: int, d_gamma: int, d_beta: int,
                           d_mean_rstd: int, d_running_mean: int, d_running_var: int, eps: float, slope: float, training: bool, d_res: int,
                           d_bias: int, d_G: int, d_agg: int, d_grad_gamma: int, d_grad_beta: int, d_grad_b: int, stream: int = 0):
    """gat_op_batch_norm_backward on device pointers: G and agg [n_rows][H*D] from dL/dhout (d_g, or d_gh for the last layer); the
    three gradient vectors [H*D] are added into (0: not formed)."""
    p = lambda x: C.c_void_p(x or None)
    _chk(load_library().gat_op_batch_norm_backward(p(d_u), p(d_g), p(d_gh), gh_stride, n_rows, H, D, p(d_gamma), p(d_beta), p(d_mean_rstd),
                                                   p(d_running_mean), p(d_running_var), eps, slope, int(bool(training)), p(d_res), p(d_bias),
                                                   p(d_G), p(d_agg), p(d_grad_gamma), p(d_grad_beta), p(d_grad_b), p(stream)))


def op_pair_forward(d_x: int, x_stride: int, d_u: int, d_v: int, n_pairs: int, n_rows: int, width: int, mode, d_q: int, stream: int = 0):
    """gat_op_pair_forward on device pointers: q [n_pairs][width] = x[u] * x[v] ("mul") or x[u] + x[v] ("add")."""
    _chk(load_library().gat_op_pair_forward(C.c_void_p(d_x or None), x_stride, C.c_void_p(d_u or None), C.c_void_p(d_v or None), n_pairs,
                                            n_rows, width, pair_mode(mode), C.c_void_p(d_q or None), C.c_void_p(stream or None)))


def op_pair_backward(d_gq: int, d_x: int, x_stride: int, d_u: int, d_v: int, n_pairs: int, n_rows: int, width: int, mode, d_gh: int,
                     gh_stride: int, stream: int = 0):
    """gat_op_pair_backward on device pointers: floats 0..width-1 of every gh row from the pair rows' gradient (d_x may be 0 for "add")."""
    _chk(load_library().gat_op_pair_backward(C.c_void_p(d_gq or None), C.c_void_p(d_x or None), x_stride, C.c_void_p(d_u or None),
                                             C.c_void_p(d_v or None), n_pairs, n_rows, width, pair_mode(mode), C.c_void_p(d_gh or None),
                                             gh_stride, C.c_void_p(stream or None)))


def op_head_hidden_forward(d_a: int, d_b1: int, rows: int, width: int, slope: float = 0.0, stream: int = 0):
    """gat_op_head_hidden_forward on device pointers: a [rows][width] becomes act(a + b1) in place (slope 0 = ReLU)."""
    _chk(load_library().gat_op_head_hidden_forward(C.c_void_p(d_a or None), C.c_void_p(d_b1 or None), rows, width, slope, C.c_void_p(stream or None)))


def op_head_hidden_backward(d_gz: int, d_z1: int, rows: int, width: int, slope: float = 0.0, d_grad_b1: int = 0, stream: int = 0):
    """gat_op_head_hidden_backward on device pointers: gz [rows][width] becomes gz * (z1 > 0 ? 1 : slope) in place; its column sums are
    added into grad_b1 [width] (0: not formed)."""
    _chk(load_library().gat_op_head_hidden_backward(C.c_void_p(d_gz or None), C.c_void_p(d_z1 or None), rows, width, slope,
                                                    C.c_void_p(d_grad_b1 or None), C.c_void_p(stream or None)))


def op_negative_sample(d_row_ptr: int, d_col_idx: int, n_rows: int, n_edges: int, mode, flags: int, seed: int, round: int, d_u: int, d_v: int,
                       count: int, d_src_u: int = 0, d_src_v: int = 0, n_src: int = 0, stream: int = 0) -> int:
    """gat_op_negative_sample on device pointers: d_u / d_v [count] int32 receive round `round` of the sampling law on the CSR (rows =
    destinations); d_src_u / d_src_v [n_src] are the source pairs of "corrupt".  -> the unfiltered count."""
    uf = C.c_int64()
    _chk(load_library().gat_op_negative_sample(C.c_void_p(d_row_ptr or None), C.c_void_p(d_col_idx or None), n_rows, n_edges, neg_mode(mode),
                                               int(flags), int(seed) & 0xFFFFFFFFFFFFFFFF, int(round) & 0xFFFFFFFFFFFFFFFF,
                                               C.c_void_p(d_src_u or None), C.c_void_p(d_src_v or None), n_src, C.c_void_p(d_u or None),
                                               C.c_void_p(d_v or None), count, C.byref(uf), C.c_void_p(stream or None)))
    return uf.value


RANK_MAX_KS = 8
# gat_rank_stats, field for field (no padding: every member is 8 bytes wide)
RANK_STATS_DTYPE = np.dtype([("n_pos", np.int64), ("n_neg", np.int64), ("n_nan", np.int64), ("auc_num", np.uint64), ("ap", np.float64),
                             ("mrr", np.float64), ("hits", np.int64, (RANK_MAX_KS,))])


def rank_stats_dict(out: np.ndarray, n_ks: int) -> dict:
    """A gat_rank_stats array as a dict of per-column arrays, with the two ratios callers divide out themselves: auc = auc_num /
    (2 n_pos n_neg), NaN where a class is missing; hits_at = hits / n_pos (NaN without positives)."""
    d = {f: out[f].copy() for f in ("n_pos", "n_neg", "n_nan", "auc_num", "ap", "mrr")}
    d["hits"] = out["hits"][:, :n_ks].copy()
    pn = d["n_pos"].astype(np.float64) * d["n_neg"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d["auc"] = np.where(pn > 0, d["auc_num"].astype(np.float64) / (2.0 * pn), np.nan)
        d["hits_at"] = np.where(d["n_pos"][:, None] > 0, d["hits"].astype(np.float64) / d["n_pos"][:, None].astype(np.float64), np.nan)
    return d


def op_rank_stats(d_scores: int, score_stride: int, n_rows: int, n_cols: int, d_labels: int = 0, d_targets: int = 0, d_mask: int = 0,
                  ks=(), stream: int = 0) -> dict:
    """gat_op_rank_stats on device pointers: the ranking statistics per column of scores [n_rows][n_cols] (rows score_stride floats
    apart) against int32 labels [n_rows] or float targets [n_rows][n_cols] (exactly one), over the rows of the uint8 mask (0: all).
    -> the dict of GatContext.eval_rank."""
    k = np.ascontiguousarray(ks, np.int32).reshape(-1)
    out = np.zeros(max(int(n_cols), 0), RANK_STATS_DTYPE)
    _chk(load_library().gat_op_rank_stats(C.c_void_p(d_scores or None), score_stride, C.c_void_p(d_labels or None), C.c_void_p(d_targets or None),
                                          C.c_void_p(d_mask or None), n_rows, n_cols, _np_ptr(k) if len(k) else None, len(k),
                                          _np_ptr(out) if len(out) else None, C.c_void_p(stream or None)))
    return rank_stats_dict(out, len(k))


PART_BOTH, PART_LEFT, PART_RIGHT = 0, 1, 2       # the `part` of the dense seams
DENSE_SCRATCH_PROJECT, DENSE_SCRATCH_GRAD_W = 0, 1


def _p(ptr: int):
    return C.c_void_p(ptr or None)


def _dense(name: str, *args) -> str:
    """One gat_op_dense_* call on device pointers; -> the template name of the kernel the launcher picked."""
    buf = C.create_string_buffer(96)
    _chk(getattr(load_library(), name)(*args, buf, 96))
    return buf.value.decode()


def op_dense_scratch_floats(kind: int, n_rows: int, F: int, HD: int, part: int = PART_BOTH) -> int:
    out = C.c_int64()
    _chk(load_library().gat_op_dense_scratch_floats(kind, n_rows, F, HD, part, C.byref(out)))
    return out.value


def op_dense_project(d_x: int, ldx: int, d_w: int, n_rows: int, F: int, HD: int, part: int, pl_bf16: bool, d_pl: int, d_pr: int,
                     d_scratch: int = 0, scratch_floats: int = 0, stream: int = 0) -> str:
    return _dense("gat_op_dense_project", _p(d_x), ldx, _p(d_w), n_rows, F, HD, part, int(pl_bf16), _p(d_pl), _p(d_pr), _p(d_scratch),
                  scratch_floats, _p(stream))


def op_dense_grad_x(d_gpl: int, d_gpr: int, d_w: int, d_hpre_prev: int, d_gprev: int, n_rows: int, F: int, HD: int, slope: float,
                    stream: int = 0) -> str:
    return _dense("gat_op_dense_grad_x", _p(d_gpl), _p(d_gpr), _p(d_w), _p(d_hpre_prev), _p(d_gprev), n_rows, F, HD, slope, _p(stream))


def op_dense_grad_w(d_gpl: int, d_gpr: int, d_x: int, ldx: int, d_grad_w: int, d_scratch: int, scratch_floats: int, n_rows: int, F: int,
                    HD: int, part: int, stream: int = 0) -> str:
    return _dense("gat_op_dense_grad_w", _p(d_gpl), _p(d_gpr), _p(d_x), ldx, _p(d_grad_w), _p(d_scratch), scratch_floats, n_rows, F, HD,
                  part, _p(stream))


def op_dense_project_res(d_x: int, ldx: int, d_wres: int, d_r: int, n_rows: int, F: int, HD: int, stream: int = 0) -> str:
    return _dense("gat_op_dense_project_res", _p(d_x), ldx, _p(d_wres), _p(d_r), n_rows, F, HD, _p(stream))


def op_dense_grad_wres(d_g: int, d_x: int, ldx: int, d_grad_wres: int, d_scratch: int, scratch_floats: int, n_rows: int, F: int, HD: int,
                       stream: int = 0) -> str:
    return _dense("gat_op_dense_grad_wres", _p(d_g), _p(d_x), ldx, _p(d_grad_wres), _p(d_scratch), scratch_floats, n_rows, F, HD, _p(stream))


def op_dense_grad_x_res(d_g: int, d_wres: int, d_gx: int, n_rows: int, F: int, HD: int, stream: int = 0) -> str:
    return _dense("gat_op_dense_grad_x_res", _p(d_g), _p(d_wres), _p(d_gx), n_rows, F, HD, _p(stream))


def _coo_sizes(n_in: int, n_rows: int, n_table: Optional[int], flags: int) -> int:
    if int(n_in) < 0 or int(n_rows) <= 0:
        raise ValueError(f"edge list: bad sizes (n_in={n_in}, n_rows={n_rows})")
    if not isinstance(flags, (int, np.integer)) or flags < 0:
        raise TypeError("flags must be a non-negative int (GRAPH_SELF_LOOPS | GRAPH_SYMMETRIZE | GRAPH_COALESCE)")
    return int(n_rows) if n_table is None else int(n_table)


def _coo_args(src, dst, n_rows: int, n_table: Optional[int], flags: int):
    """Argument checks of the host edge-list entry points: raise before any library call."""
    s, d = np.asarray(src), np.asarray(dst)
    for name, a in (("src", s), ("dst", d)):
        if a.ndim != 1:
            raise ValueError(f"{name} must be one-dimensional, got shape {a.shape}")
        if a.size and a.dtype.kind not in "iu":
            raise TypeError(f"{name} must hold integers, got {a.dtype}")
        if a.size and (int(a.max()) > 0x7fffffff or int(a.min()) < -0x80000000):
            raise ValueError(f"{name} does not fit int32")
    if len(s) != len(d):
        raise ValueError(f"src and dst differ in length ({len(s)} vs {len(d)})")
    nt = _coo_sizes(len(s), n_rows, n_table, flags)
    return np.ascontiguousarray(s, np.int32), np.ascontiguousarray(d, np.int32), nt


def graph_from_coo(src, dst, n_rows: int, n_table: Optional[int] = None, table_row0: int = 0, flags: int = 0, device: int = 0):
    """Edge list (host arrays; a message flows src -> dst) -> (row_ptr, col_idx) int32, built on the device: rows are
    destinations, sources ascending inside a row.  flags: GRAPH_SELF_LOOPS | GRAPH_SYMMETRIZE | GRAPH_COALESCE, applied
    in that order (gatv2_abi.h "graph construction").  Does the count-then-fill pair of calls."""
    s, d, nt = _coo_args(src, dst, n_rows, n_table, flags)
    lib = load_library()
    m = C.c_int64()
    _chk(lib.gat_graph_from_coo(_np_ptr(s), _np_ptr(d), len(s), n_rows, nt, table_row0, flags, None, None, 0, C.byref(m), device))
    rp, ci = np.empty(n_rows + 1, np.int32), np.empty(m.value, np.int32)
    _chk(lib.gat_graph_from_coo(_np_ptr(s), _np_ptr(d), len(s), n_rows, nt, table_row0, flags, _np_ptr(rp), _np_ptr(ci), m.value,
                                C.byref(m), device))
    return rp, ci


def graph_from_coo_device(d_src: int, d_dst: int, n_in: int, n_rows: int, n_table: Optional[int] = None, table_row0: int = 0,
                          flags: int = 0, d_row_ptr: int = 0, d_col_idx: int = 0, col_capacity: int = 0, stream: int = 0) -> int:
    """The stateless builder on device pointers (current device).  Returns the edge count of the result; with d_col_idx == 0
    that is all it does, otherwise d_row_ptr [n_rows+1] and d_col_idx [col_capacity] are filled (too small: GatError, and the
    needed count is in its `needed` attribute)."""
    nt = _coo_sizes(n_in, n_rows, n_table, flags)
    m = C.c_int64(-1)
    rc = load_library().gat_graph_from_coo_device(C.c_void_p(d_src or None), C.c_void_p(d_dst or None), n_in, n_rows, nt, table_row0,
                                                  flags, C.c_void_p(d_row_ptr or None), C.c_void_p(d_col_idx or None), col_capacity,
                                                  C.byref(m), C.c_void_p(stream or None))
    if rc != 0:
        err = GatError(rc, load_library().gat_last_error().decode("utf-8", "replace"))
        err.needed = m.value if m.value >= 0 else None
        raise err
    return m.value


def graph_check_device(d_row_ptr: int, d_col_idx: int, n_rows: int, n_edges: int, n_table: Optional[int] = None, stream: int = 0):
    """One pass over a device CSR: (problem, where) — (CSR_OK, -1) or the first broken rule and the lowest offending index."""
    nt = int(n_rows) if n_table is None else int(n_table)
    prob, where = C.c_int32(), C.c_int64()
    _chk(load_library().gat_graph_check_device(C.c_void_p(d_row_ptr or None), C.c_void_p(d_col_idx or None), n_rows, n_edges, nt,
                                               C.byref(prob), C.byref(where), C.c_void_p(stream or None)))
    return prob.value, where.value


def mem_info():
    lib = load_library()
    f, t = C.c_size_t(), C.c_size_t()
    _chk(lib.gat_mem_info(C.byref(f), C.byref(t)))
    return f.value, t.value


def device_count() -> int:
    lib = load_library()
    n = C.c_int()
    _chk(lib.gat_device_count(C.byref(n)))
    return n.value
