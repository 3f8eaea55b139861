"""The sizes at which the loss-term kernels (ml-neuman_amd/csrc/loss.hip) and the image-metric kernels (ml-neuman_amd/csrc/frame.hip) change
behaviour, and the sizes tests/test_hip_loss_edges.py and tests/test_hip_frame_edges.py cross them with.

TABLE has the form of tests/helpers/component_sizes.py's: name -> (value, source file, pattern whose integer groups multiply to the value);
tests/test_loss_host.py checks on the CPU that every entry still reads so in the source and that every derived size lies past the threshold it
claims, so that a retune fails there instead of silently un-crossing an edge."""
import types

CSRC = 'ml-neuman_amd/csrc/'
TABLE = {
    # every loss kernel: a grid-stride loop of at most kLossMaxBlocks workgroups of kLossThreads
    'LOSS_THREADS': (256, CSRC + 'loss.hip', r'constexpr int kLossThreads = (\d+);'),
    'LOSS_MAX_BLOCKS': (1024, CSRC + 'loss.hip', r'constexpr int kLossMaxBlocks = (\d+);'),
    # the workspace: six doubles per workgroup (the shape prior's three sums and three counts)
    'LOSS_WS_PER_BLOCK': (6, CSRC + 'loss.hip', r'return \(int64_t\)kLossMaxBlocks \* (\d+);'),
    # wave_total: one wave of this many lanes adds the partials, lane l takes l, l + 64, ...
    'FINISH_LANES': (64, CSRC + 'loss.hip', r'for \(int i = threadIdx\.x; i < blocks; i \+= (\d+)\) s \+= partial'),
    # nm_ssd_u8: a workgroup is sized for 256 x 16 bytes, the grid is capped
    'SSD_PER_BLOCK': (4096, CSRC + 'frame.hip', r'const int64_t blocks = \(n \+ (\d+) \* (\d+) - 1\) / \(256 \* 16\);'),
    'SSD_THREADS': (256, CSRC + 'frame.hip', r'const int64_t blocks = \(n \+ (\d+) \* 16 - 1\)'),
    'SSD_MAX_BLOCKS': (4096, CSRC + 'frame.hip', r'dim3\(\(unsigned\)\(blocks < (\d+) \? blocks : 4096\)\)'),
    # nm_ssim_u8: one thread per (pixel of the cropped image, channel), 256 per workgroup, one partial per workgroup
    'SSIM_WIN': (7, CSRC + 'frame.hip', r'constexpr int kSsimWin = (\d+), kSsimPad = 3;'),
    'SSIM_THREADS': (256, CSRC + 'frame.hip', r'ssim_partial_kernel, dim3\(blocks\), dim3\((\d+)\)'),
    'SSIM_MAX_BLOCKS': (4096, 'include/neuman_hip.h', r'#define NM_SSIM_WORKSPACE_DOUBLES (\d+)'),
}
C = types.SimpleNamespace(**{k: v[0] for k, v in TABLE.items()})

# ---- loss --------------------------------------------------------------------------------------------------------------------------------
SWEEP = C.LOSS_THREADS * C.LOSS_MAX_BLOCKS                     # 262 144 items: what one pass of the grid covers
WORKSPACE_DOUBLES = C.LOSS_MAX_BLOCKS * C.LOSS_WS_PER_BLOCK
PAIR_SWEEP_SIZES = (SWEEP, SWEEP + 1, SWEEP + C.LOSS_THREADS + 1, 2 * SWEEP + 3)
# (nh, nd): the sums kernel's grid follows max(nh, nd), the gradient kernel's nh + nd and switches arrays at item nh
SHAPE_SWEEP_SIZES = ((SWEEP + 1, 5), (5, SWEEP + 1), (SWEEP // 2 + 1, SWEEP // 2 + 1), (2 * SWEEP + 3, 0), (700, 0))
BLOCK_COUNTS = (1, C.FINISH_LANES - 1, C.FINISH_LANES, C.FINISH_LANES + 1)
BLOCK_COUNT_SIZES = tuple(s for k in BLOCK_COUNTS for s in (C.LOSS_THREADS * k, C.LOSS_THREADS * k + 1))
EDGE_SIZES = (4099, SWEEP + C.LOSS_THREADS + 1)
LARGEST = 2 * SWEEP + 3


def loss_blocks(n):
    return max(1, min(C.LOSS_MAX_BLOCKS, (n + C.LOSS_THREADS - 1) // C.LOSS_THREADS))


def sweeps(n):
    """the passes of the grid-stride loop that the busiest thread makes over n items"""
    return (n + SWEEP - 1) // SWEEP


def planted_edges(n):
    """the row boundaries the edge table is planted across: the start, the first workgroup's end, one sweep, the end -- those that fit in n"""
    return tuple(b for b in (0, C.LOSS_THREADS, SWEEP, n) if b <= n)


# ---- frame -------------------------------------------------------------------------------------------------------------------------------
SSD_SWEEP = C.SSD_PER_BLOCK * C.SSD_MAX_BLOCKS                 # 16 777 216 bytes: the grid cap of nm_ssd_u8
SSD_STRIDE = C.SSD_THREADS * C.SSD_MAX_BLOCKS                  # what one pass of the capped grid covers: each thread makes 16 of them
SSD_SIZES_SMALL = (1, C.SSD_PER_BLOCK - 1, C.SSD_PER_BLOCK, C.SSD_PER_BLOCK + 1)
SSD_SIZES_CAP = (SSD_SWEEP, SSD_SWEEP + 1)
SSD_PAST_THE_CAP = SSD_SWEEP + C.SSD_THREADS + 1
SSIM_SWEEP = C.SSIM_THREADS * C.SSIM_MAX_BLOCKS                # 1 048 576 (pixel, channel) items
SSIM_SHAPES = ((7, 7, 1), (7, 300, 3), (300, 7, 3), (31, 45, 2), (31, 45, 4), (600, 600, 3), (850, 850, 3))
BYTE_SIZES = (1, 255, 256, 257)


def ssim_items(shape):
    H, W, Ch = shape
    return (H - C.SSIM_WIN + 1) * (W - C.SSIM_WIN + 1) * Ch
