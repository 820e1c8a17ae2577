"""Thin Python layer over the C ABI: device buffers (torch on the GPU), contexts and frame streams, one module per concern.

PyTorch is plumbing only (device memory + streams); all arithmetic happens in liblecturemath_hip.so.
With the test-only emulated library (tests/hipemu) "device" memory is host memory and numpy arrays
stand in for torch tensors; the product never selects that path by itself (see _lib.load).

The names below are the package's surface; callers import them from here, not from the modules.
"""
from ._base import Backend
from .labeling import FrameLabeler, frame_sums
from .segment import ConflictSignal, image_pairs_overlap
from .group_images import GroupImages, LazyGroupImages, _LazyImageList, decode_crop
from .history import FrameHistory, as_frame_history
from .align import ALIGN_MAX_WINDOW, TranslationAligner
from .pair_counts import CC_PAIR_MAX_RADIUS, CCPairCounts, PairTableView, _PairCounts
from .keyframe_ccs import KeyframeCCs, _plain_cc, device_cc_class, pixel_sums
from .stream import _G_DTYPES, _G_NAMES, FrameStream, Grouping
