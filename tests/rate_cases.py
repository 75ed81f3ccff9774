"""What tests/test_dropout_rates_cpu.py and tests/test_gpu_dropout_rates.py share: the table of every dropout site of the C ABI,
the rates and shapes the GPU file runs, and the count of elements on which the two keep rules differ.  Plain module (not a
conftest): numpy only, no GPU.

Three threshold widths coexist in the kernels:
  *  8 bit: keep iff byte >= thr8 = round(256 p); realised rate thr8 / 256; scale 256 / (256 - thr8);
  * 16 bit: keep iff half-word >= floor(65536 p); scale 1 / (1 - p) -- ops feeds it thr8 / 256, where both are exact;
  * 24 bit: keep iff u = (word >> 8) / 2^24 >= p (float32); scale 1 / (1 - p).
On a 24-bit stream the 8-bit rule is `u >= thr8 / 256` (the top byte of u against thr8), so `band()` below counts the elements
the two rules treat differently: those with u between p and thr8 / 256.  At p = 0.25 and 0.5 there are none, and the two scales
are the same number: a site that draws under one width and scales under the other, or a backward that regenerates its gate
under the other width, is invisible there.
"""
import dropout_replay as R

# round(256 p): 26 (realised 0.1016, above p), 51 (0.1992, below p), 64 and 128 (exact)
RATES = (0.1, 0.2, 0.5, 0.25)
INEXACT = (0.1, 0.2)
SMALL = 0.001                        # round(256 p) = 0: an 8-bit site realises no dropout, a 24-bit site still drops

# shapes of the GPU file (tests/test_gpu_dropout_rates.py)
ENCODER = dict(nb=2, ns=5, T=6, d=256)            # mha_small: every site on the 24-bit stream
ENCODER_LONG = dict(nb=1, ns=1, T=17, d=256)      # attention probabilities on the 8-bit block hash, the rest 24 bit
POOL_SHAPES = ((6, 32), (65, 1))                  # (L, ns), two branches, d = 256
POOL_PAIRS = ((0.1, 0.2), (0.2, 0.1))             # (p_head, p_rho)
SNN_NS = 5
MAP_LENGTHS = ([33, 5], [777])
MAP_N_Q = 6
# the stream the K2 map cases pin: at this offset the 228-element map of [33, 5] has an element in the band at 0.1 and at 0.2
# (most offsets have none: 228 x 1.6e-3); asserted by the CPU file
MAP_OFF = 7000
PATCH_ROWS = 3000


def thr8(p: float) -> int:
    return int(p * 256.0 + 0.5)


def realised(p: float) -> float:
    return thr8(p) / 256.0


def scale8(p: float) -> float:
    return 256.0 / (256.0 - thr8(p))


def scale24(p: float) -> float:
    return 1.0 / (1.0 - p)


def band(seed: int, off: int, n: int, p: float) -> int:
    """Elements 0 .. n-1 of the stream at `off` that the 24-bit rule at p and the 8-bit rule at round(256 p) treat differently."""
    return int((R.kept(seed, off, n, p) != R.kept(seed, off, n, realised(p))).sum())


def keeps_under_8bit_rule(p: float) -> float:
    """The rate to hand dropout_replay's *_keeps functions to get a 24-bit site's masks as the 8-bit rule would draw them:
    other dropped elements inside the band, and the scale 1 / (1 - thr8 / 256) = 256 / (256 - thr8)."""
    return realised(p)


# ------------------------------------------------------------------------------------------- the site table
# entry -> (parameter(s) that carry the rate or the keep scale, width, scale, the GPU test that runs it at p != 0.25)
# width: 8 / 16 / 24 as above; "8+24": the encoder's attention probabilities take the 8-bit block hash for T > 16 and the
# 24-bit stream up to 16, every other site of the entry the 24-bit stream; "scale": the entry draws nothing -- it is handed a
# keep scale (or the rate to form one from) and gates by the zeros of the H_bag it reads.
S8, S16, S24 = "256 / (256 - round(256 p))", "1 / (1 - p), p = round(256 p) / 256 from ops", "1 / (1 - p)"
GPU_FILE = "test_gpu_dropout_rates.py"
STEP = "test_whole_step_gives_every_site_its_own_rate"
PATCH, ENC, POOL, SNN, MAP, BIL = ("test_patch_layer_routes_hold_the_realised_scale", "test_encoder_rates_equal_fp64_oracle",
                                   "test_pool_head_and_rho_rates_equal_fp64_oracle", "test_omic_snn_rates_equal_fp64_oracle",
                                   "test_k2_map_rates_mask_scale_and_fp64_oracle", "test_bilinear_head_rate_equals_fp64_oracle")
SITES = {
    "mpo_patch_fc_forward": (("drop_p",), "8", S8, PATCH),
    "mpo_patch_fc_f32_forward": (("drop_p",), "8", S8, PATCH),
    "mpo_patch_fc_f32_forward_dev": (("drop_p",), "8", S8, PATCH),
    "mpo_patch_coattn_mcat_forward": (("drop_p",), "8", S8, PATCH),
    # (the benchmark's roofline leg: mpo_patch_fc_forward's launcher and kernel without the weight packing; no test calls it
    #  in training mode -- its check and kernel are the ones the patch-layer test runs)
    "mpo_patch_coattn_fwd_bagpass": (("drop_p",), "8", S8, PATCH),
    "mpo_patch_epilogue_forward": (("drop_p",), "16", S16, PATCH),
    "mpo_patch_epilogue_backward": (("drop_p",), "scale", S16, PATCH),
    "mpo_patch_fc_f32_backward": (("gate",), "scale", S8, PATCH),
    "mpo_coattn_mcat_backward": (("bag_relu_gate",), "scale", S8, PATCH),
    # (NaCAGaT on a bf16 window: the medium model's key route picks one of the two; both take the same gate argument)
    "mpo_nacagat_patch_grad": (("relu_gate",), "scale", S8, STEP),
    "mpo_nacagat_patch_grad_fused": (("relu_gate",), "scale", S8, STEP),
    "mpo_bag_self_attention_forward": (("drop_p",), "8", S8 + ", round(256 p) clamped at 255",
                                       "test_gpu_bag_selfattn_edges.py::test_dropout_rate_is_quantised_and_sequences_draw_their_own_masks"),
    "mpo_bag_self_attention_backward": (("drop_p",), "8", S8 + ", round(256 p) clamped at 255",
                                        "test_gpu_bag_selfattn_edges.py::test_dropout_rate_is_quantised_and_sequences_draw_their_own_masks"),
    "mpo_encoder_forward": (("drop_p",), "8+24", S24 + "; attention probabilities for T > 16: " + S8, ENC),
    "mpo_encoder_backward": (("drop_p",), "8+24", S24 + "; attention probabilities for T > 16: " + S8, ENC),
    "mpo_gated_pool_forward": (("head_drop_p", "rho_drop_p"), "24", S24, POOL),
    "mpo_gated_pool_backward": (("head_drop_p", "rho_drop_p"), "24", S24, POOL),
    "mpo_omic_snn_forward": (("drop_p",), "24", "AlphaDropout: a (keep ? x : alpha') + b, a and b functions of p", SNN),
    "mpo_omic_snn_backward": (("drop_p",), "24", "AlphaDropout: the kept elements' derivative is a(p)", SNN),
    "mpo_coattn_nacagat_forward": (("drop_p",), "24", S24, MAP),
    "mpo_coattn_nacagat_backward": (("drop_p",), "24", S24, MAP),
    "mpo_bilinear_head_forward": (("drop_p",), "24", S24, BIL),
    "mpo_bilinear_head_backward": (("drop_p",), "24", S24, BIL),
    "mpo_bilinear_head_loss_forward": (("drop_p",), "24", S24, BIL),
    "mpo_bilinear_head_loss_backward": (("drop_p",), "24", S24, BIL),
}
# float parameters of the public headers that carry a dropout rate or a keep scale, decided from include/*.h: every rate is
# spelled drop_p, head_drop_p or rho_drop_p there; p, p_head and p_rho are the spellings of the kernels and of ops, listed so a
# new entry that uses them is caught too; the three gate spellings carry 1 / (1 - realised rate) into a backward.
RATE_NAMES = {"p", "drop_p", "p_head", "p_rho", "head_drop_p", "rho_drop_p", "dropout", "dropout_p", "p_drop"}
SCALE_NAMES = {"gate", "relu_gate", "bag_relu_gate", "keep_scale", "inv_keep"}
# the other float parameters the headers have today: none of them is a rate.  A float parameter outside the three sets fails
# the CPU test until someone says which it is.
OTHER_FLOATS = {"alpha", "eps", "l1", "max_norm", "lr", "beta1", "beta2", "weight_decay", "x_scale"}
