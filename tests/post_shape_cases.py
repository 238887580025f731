"""The case table of tests/test_post_shapes_host.py (no GPU) and tests/test_gpu_post_shapes.py: the shapes at which the
post-processor's kernels (mdp_playground_amd/csrc/mdpp_post.hip) take another path, and a pure-Python statement of the
kernel form each case must get -- what VectorPostProcessor.kernel_name() is asserted against on the GPU.

The statement is written from the kernels' documentation, not from their code: the LDS form of the picture kernel stages
one source picture transposed, a row per source column at an odd dword pitch with one spare dword, and needs whole
dwords on both sides."""
import sys

import numpy as np

K_BLOCK = 256               # lanes per workgroup
PASS_DWORDS = K_BLOCK * 8   # dwords k_post_image_lds stages / writes per pass of its two loops
LDS_LIMIT = 60 * 1024       # above it a handle gets the general picture kernel
GENERAL_MAX_BLOCKS = 65536  # the general picture kernel's grid cap (beyond it: its grid-stride loop)
NUM_CUS = 256               # MI355X
PRE = 8                     # reward / done rows k_post_step keeps in flight per lane
MAX_DELAY = 128


# ---------------------------------------------------------------------------------------------------------------
# expected forms
def lds_bytes(hw, ch):
    """Dynamic LDS of k_post_image_lds for a hw x hw x ch picture, before rounding up to 16."""
    pitch = ((((hw * ch + 3) // 4) + 2) | 1) * 4
    return hw * pitch


def image_form(hw, ch, pad):
    """(kernel, lds bytes, workgroups per CU) of a picture handle; the general kernel has no LDS and no tier."""
    th = hw + 2 * pad
    whole_dwords = (hw * ch) % 4 == 0 and (th * ch) % 4 == 0        # source rows and canvas rows
    fits_table = th * ch < 65536 and th < 16384 and ch <= 16        # 16 bits of row byte, 14 of x, 4 of c
    raw = lds_bytes(hw, ch)
    if not (whole_dwords and fits_table and raw <= LDS_LIMIT):
        return "k_post_image", 0, 0
    lds = (raw + 15) & ~15
    return "k_post_image_lds", lds, (2 if lds > 40 * 1024 else 4 if lds > 24 * 1024 else 6)


def image_name(hw, ch, pad):
    kernel, lds, per_cu = image_form(hw, ch, pad)
    return kernel if kernel == "k_post_image" else f"{kernel}<LDS={lds},PER_CU={per_cu}>"


def step_form(delay):
    """(RING, DC) of k_post_step: 2 = register FIFO with the delay as a constant, 1 = LDS ring, 0 = HBM slots / none."""
    if 1 <= delay <= 8:
        return 2, delay
    return (1, 0) if 9 <= delay <= 16 else (0, 0)


def step_name(rng, delay):
    ring, dc = step_form(delay)
    return f"k_post_step<PHILOX={int(rng == 'philox')},RING={ring},DC={dc}>"


def kernel_name(rng, delay, image=None):
    """image = (hw, ch, pad) or None."""
    return step_name(rng, delay) + ("" if image is None else " + " + image_name(*image))


# ---------------------------------------------------------------------------------------------------------------
# pictures.  Every case: reset, then two fused calls of K steps on N instances, done steps under autoreset=True.
# pad None: the wrapper's default image_padding (20); shq None: its default image_sh_quant (1).
def _pic(name, hw, ch, pad, N, K, *, tr="shift", shq=None, rngs=("numpy",), delay=1, form, lds=0, per_cu=0, tags=()):
    return dict(name=name, hw=hw, ch=ch, pad=pad, N=N, K=K, tr=tr, shq=shq, rngs=tuple(rngs), delay=delay,
                form=form, lds=lds, per_cu=per_cu, tags=frozenset(tags))


LDS, GEN = "k_post_image_lds", "k_post_image"
PICTURES = [
    # the reference's picture size on its default canvas; image_sh_quant 4 as in the golden w_img_84
    _pic("84x84x3_pad20_q4", 84, 3, None, 65, 3, shq=4, rngs=("numpy", "philox"), form=LDS, lds=21840, per_cu=6,
         tags=("tier6", "multipass", "ragged_pass")),
    # ... and with every shift: top * C takes every residue mod 4 (the funnel shift's rel & 3 = 1, 2, 3)
    _pic("84x84x3_pad20_q1", 84, 3, None, 33, 2, form=LDS, lds=21840, per_cu=6, tags=("tier6", "multipass", "ragged_pass", "funnel")),
    _pic("84x84x1_pad20", 84, 1, None, 33, 2, form=LDS, lds=7728, per_cu=6, tags=("tier6",)),
    _pic("100x100x3_pad20", 100, 3, None, 24, 2, form=LDS, lds=30800, per_cu=4, tags=("tier4", "multipass", "ragged_pass")),
    _pic("120x120x3_pad4", 120, 3, 4, 24, 2, form=LDS, lds=44640, per_cu=2, tags=("tier2", "multipass")),
    _pic("128x128x3_pad2", 128, 3, 2, 24, 2, form=LDS, lds=50688, per_cu=2, tags=("tier2", "over48k", "multipass")),
    _pic("140x140x3_pad2", 140, 3, 2, 24, 2, form=LDS, lds=59920, per_cu=2, tags=("tier2", "over48k", "largest_lds")),
    _pic("144x144x3_pad2_q5", 144, 3, 2, 24, 2, shq=5, form=GEN, tags=("past_lds_limit", "quant_over_pad")),
    _pic("84x84x3_pad1", 84, 3, 1, 24, 2, form=GEN, tags=("ragged_canvas_row",)),
    _pic("2x2x2_pad1", 2, 2, 1, 257, 3, form=LDS, lds=32, per_cu=6, tags=("smallest_lds",)),
    _pic("2x2x1_pad1", 2, 1, 1, 257, 3, form=GEN, tags=("smallest_general",)),
    _pic("6x6x2_pad1", 6, 2, 1, 65, 3, form=LDS, lds=128, per_cu=6),
    _pic("32x32x4_pad3_q2", 32, 4, 3, 64, 2, shq=2, form=LDS, lds=4480, per_cu=6),
    _pic("8x8x16_pad2_q3", 8, 16, 2, 64, 2, shq=3, form=LDS, lds=1120, per_cu=6, tags=("c16", "quant_over_pad")),
    _pic("8x8x17_pad2", 8, 17, 2, 64, 2, form=GEN, tags=("c_over_16",)),
    _pic("12x12x3_flip_pad0", 12, 3, 0, 64, 2, tr="flip", form=LDS, lds=528, per_cu=6, tags=("no_draw",)),
    # image_sh_quant above the padding: the shift is drawn and always truncates to 0
    _pic("16x16x3_pad2_q5", 16, 3, 2, 64, 2, shq=5, form=LDS, lds=960, per_cu=6, tags=("quant_over_pad",)),
    # picture counts
    _pic("one_84x84x3_pad20", 84, 3, None, 1, 1, form=LDS, lds=21840, per_cu=6, tags=("one",)),
    _pic("one_84x84x3_pad1", 84, 3, 1, 1, 1, form=GEN, tags=("one",)),
    _pic("wrap_16x16x3_pad2", 16, 3, 2, 520, 3, form=LDS, lds=960, per_cu=6, tags=("lds_wrap",)),
    _pic("wrap_128x128x3_pad2", 128, 3, 2, 260, 2, form=LDS, lds=50688, per_cu=2, tags=("lds_wrap", "over48k")),
    # 2 x 3102 canvases of 22 188 bytes (138 MB) and 1034 at the reset, every one compared
    _pic("wrap_84x84x3_pad1", 84, 3, 1, 1034, 3, form=GEN, tags=("general_wrap",)),
]
PICTURE = {p["name"]: p for p in PICTURES}
# masked reset with out= holding the previous canvases, once per picture kernel
MASKED_RESET = ["84x84x3_pad20_q1", "84x84x3_pad1"]


def pic_pad(p):
    return 20 if p["pad"] is None else p["pad"]


def pic_config(p):
    """(wrapper config keys, PostOracle keywords) of a picture case."""
    cfg = dict(image_transforms=p["tr"])
    if p["pad"] is not None:
        cfg["image_padding"] = p["pad"]
    if p["shq"] is not None:
        cfg["image_sh_quant"] = p["shq"]
    okw = dict(cfg, image_shape=(p["hw"], p["hw"], p["ch"]))
    return cfg, okw


def canvas_dwords(p):
    th = p["hw"] + 2 * pic_pad(p)
    return th * th * p["ch"] // 4


def source_dwords(p):
    return p["hw"] * p["hw"] * p["ch"] // 4


def general_blocks(p, pictures):
    return (pictures * canvas_dwords(p) + K_BLOCK - 1) // K_BLOCK


# ---------------------------------------------------------------------------------------------------------------
# numpy restatement of get_transformed_image (gym_env_wrapper.py:523-618): draw, truncate, paste, transpose
def np_place(gen, hw, pad, shift, shq):
    tot = hw + 2 * pad
    sw = sh = tot // 2
    if shift:
        m = (tot - hw) // 2
        aw = int(gen.integers(-m + 1, m))
        ah = int(gen.integers(-m + 1, m))
        sw += int(aw / shq) * shq
        sh += int(ah / shq) * shq
    return sh - hw // 2, sw - hw // 2           # top, left


def np_picture(gen, img, pad, shift, shq):
    hw, _, ch = img.shape
    tot = hw + 2 * pad
    top, left = np_place(gen, hw, pad, shift, shq)
    canvas = np.zeros((tot, tot, ch), np.uint8)
    canvas[top:top + hw, left:left + hw] = img
    return np.ascontiguousarray(canvas.transpose(1, 0, 2))


def wrapper_generator(seed):
    """Instance `seed`'s generator as the wrapper's constructor leaves it: two space seeds drawn (:102-103)."""
    from mdp_playground_amd import mdp as mdp_mod
    g = mdp_mod.new_generator(int(seed))
    for _ in range(2):
        g.integers(sys.maxsize)
    return g


# ---------------------------------------------------------------------------------------------------------------
# step and action kernels
SEED, ENV0 = 77, 500                    # config seed (numpy: instance i is seeded SEED + ENV0 + i) and env_id_offset
RING_DELAYS = [0, 1, 7, 8, 9, 16, 17, 128]
RING_CALLS = [7, 8, 17]                 # three fused calls
RING_N = 257
REFUSED_DELAY = 129
REFUSAL = "need 0 <= delay <= 128"
FLUSH_DELAYS = [7, 8, 9, 16, 17, 127, 128]
K_SEQUENCE = [1, 7, 8, 9, 15, 16, 17]   # around the prefetch depth, one handle in sequence
K_SEQUENCE_DELAYS = [3, 40]             # register ring, HBM ring
N_CASES = [1, 63, 64, 65, 255, 256, 257, 1000]
NO_AUTORESET_DELAYS = [5, 12, 33]       # register, LDS and HBM rings
CONT_DIMS = [1, 3, 17]
CONT_NOISES = [0.2, 0.0, None]          # None: the key is absent
ACTION_COUNTS = [2, 6, 64, 300]
ACTION_NOISES = [0.0, 0.25, 1.0]
RNGS = ["numpy", "philox"]
