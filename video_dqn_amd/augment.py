"""Random shift and left-right mirror augmentation of the training minibatch, fused into the input pack.

The reference shows the network every frame as the same 224 x 224 centre crop (``Resize + CenterCrop + Normalize``,
util/torch.py:5-12).  With ``AUG_SHIFT_PAD`` > 0 and / or ``AUG_FLIP`` the trainer draws one ``(sx, sy, flip)`` per update and
per sample on the device — shared by the sample's frames and by s and s', because the action label is the camera motion between
the two — and the engine packs the frames through ``vdqn_pack_input_aug``: mirror the source, pad it by edge replication, crop
at the drawn offset.  Both are index remaps of uint8 pixels, so the stem operand equals ``vdqn_pack_input`` of the augmented
frames bit for bit (video_dqn_amd/csrc/augment.hip has the arithmetic, tests/aug_oracle.py restates it in numpy).  A mirrored
sample's action label has ``AUG_FLIP_ACTIONS`` exchanged (a left turn becomes a right turn).  Three small launches and no host
round trip per update.

Colour jitter (``AUG_BRIGHTNESS``, ``AUG_CONTRAST``, ``AUG_SATURATION``: the half-width J of a uniform factor range [1 - J, 1 + J],
as torchvision's ``ColorJitter``) is the photometric half: one ``(f_b, f_c, f_s)`` in Q8 per update and per sample from a stream of
its own, shared by the sample's frames and by s and s', applied as a map from uint8 pixels to uint8 pixels in integer arithmetic —
saturation, then brightness, then contrast about mid-grey 128 — inside the same pack launch (``vdqn_pack_input_aug_color``), so the
operand still equals ``vdqn_pack_input`` of host-augmented frames bit for bit (tests/aug_color_oracle.py).  One more small launch
per update.

Random zoom (``AUG_ZOOM``: J in [0, 0.5], ``AUG_ZOOM_ASPECT``) is the scale axis, a change of focal length: a window whose side is uniform
in [1 - J, 1] of the frame's (the two sides independently with ``AUG_ZOOM_ASPECT``), at a uniform position inside the frame, resampled
back to 224 x 224 — never a zoom-out.  One ``{ax, ay, bx, by}`` (Q16 step and origin) per update and per sample from a stream of its
own, shared by the sample's frames and by s and s'.  The resample is bilinear in integer arithmetic on the uint8 pixels (Q16
coordinates, Q8 weights), applied to the shifted / mirrored frame and in front of the colour transform, inside one pack launch
(``vdqn_pack_input_aug_zoom``), so the operand still equals ``vdqn_pack_input`` of host-augmented frames bit for bit
(tests/aug_zoom_oracle.py).  One more small launch per update.

Random rotation (``AUG_ROTATE``: J in [0, 30] degrees) is camera roll: an angle uniform in [-J, J] about the picture's centre, one per update
and per sample from a stream of its own, shared by the sample's frames and by s and s'.  The draw composes it with the sample's zoom row
(the identity without zoom) into one affine row ``{axx, axy, bx, 0, ayx, ayy, by, 0}`` (Q16), with sine and cosine from an integer
polynomial, and ``vdqn_pack_input_aug_affine`` resamples with the zoom's integer bilinear on 2-D tiles, so the operand still equals
``vdqn_pack_input`` of host-augmented frames bit for bit (tests/aug_rotate_oracle.py).  The affine rows reach an update as frames the
stepper packs itself (``TDStepper.step(augment_affine=)``), not through ``vdqn_step_args``.

Data parallelism keeps N ranks == one process on the big batch: every rank draws its slice of the one global draw.
"""
from __future__ import annotations

import torch

from . import _lib

MAX_PAD = 32  # vdqn_aug_draw (include/vdqn.h)
COLOR_KEYS = ("AUG_BRIGHTNESS", "AUG_CONTRAST", "AUG_SATURATION")  # the order of the factors in a colour row
MAX_ROTATE = 30.0  # vdqn_aug_draw_rotate: the angle is drawn from [-J, J] degrees, J at most 30
MAX_ZOOM = 0.5  # vdqn_aug_draw_zoom: the window's side is at least half the frame's (a magnification of 2 at the most)


def jq(j: float) -> int:
    """The Q8 half-width vdqn_aug_draw_color takes: int(J * 256 + 0.5), 0 .. 256 for J in [0, 1]."""
    return int(float(j) * 256 + 0.5)


def jz(j: float) -> int:
    """The Q16 width vdqn_aug_draw_zoom takes: int(J * 65536 + 0.5), 0 .. 32768 for J in [0, 0.5]."""
    return int(float(j) * 65536 + 0.5)


def jr(j: float) -> int:
    """The angle range vdqn_aug_draw_rotate takes, in 1 / 64 degree: int(J * 64 + 0.5), 0 .. 1920 for J in [0, 30]."""
    return int(float(j) * 64 + 0.5)


def check_config(pad, flip, flip_actions, brightness=0.0, contrast=0.0, saturation=0.0, zoom=0.0, zoom_aspect=False, rotate=0.0) -> None:
    """Raise ValueError, naming the config key, for values the augmentation does not take (host only: no device work)."""
    if isinstance(rotate, bool) or not isinstance(rotate, (int, float)) or not 0 <= rotate <= MAX_ROTATE:  # (NaN fails both comparisons)
        raise ValueError(f"AUG_ROTATE must be a number of degrees in [0, {MAX_ROTATE:g}] (0 = off: the angle is drawn from [-AUG_ROTATE, "
                         f"AUG_ROTATE]), got {rotate!r}")
    if isinstance(zoom, bool) or not isinstance(zoom, (int, float)) or not 0 <= zoom <= MAX_ZOOM:  # (NaN fails both comparisons)
        raise ValueError(f"AUG_ZOOM must be a number in [0, {MAX_ZOOM}] (0 = off: the window's side is drawn from [1 - AUG_ZOOM, 1] of the "
                         f"frame's), got {zoom!r}")
    if not isinstance(zoom_aspect, bool):
        raise ValueError(f"AUG_ZOOM_ASPECT must be True or False (got {zoom_aspect!r})")
    if zoom_aspect and jz(zoom) == 0:
        raise ValueError(f"AUG_ZOOM_ASPECT is True, but AUG_ZOOM is {zoom!r}: there is no window to stretch (set AUG_ZOOM > 0)")
    for key, j in zip(COLOR_KEYS, (brightness, contrast, saturation)):
        if isinstance(j, bool) or not isinstance(j, (int, float)) or not 0 <= j <= 1:  # (NaN fails both comparisons)
            raise ValueError(f"{key} must be a number in [0, 1] (0 = off: the factor is drawn from [1 - {key}, 1 + {key}]), got {j!r}")
    if isinstance(pad, bool) or not isinstance(pad, int) or not 0 <= pad <= MAX_PAD:
        raise ValueError(f"AUG_SHIFT_PAD must be an integer in [0, {MAX_PAD}] (got {pad!r})")
    if not isinstance(flip, bool):
        raise ValueError(f"AUG_FLIP must be True or False (got {flip!r})")
    fa = list(flip_actions) if isinstance(flip_actions, (list, tuple)) else None
    if (fa is None or len(fa) != 2 or any(isinstance(a, bool) or not isinstance(a, int) for a in fa)
            or fa[0] == fa[1] or not all(0 <= a <= 2 for a in fa)):
        raise ValueError(f"AUG_FLIP_ACTIONS must be two different actions out of 0, 1, 2 (got {flip_actions!r})")


def _u64(v: int) -> int:
    return int(v) & (2**64 - 1)


def _draw(entry: str, seed: int, step: int, global_batch: int, first: int, n: int, scalars, device, out) -> torch.Tensor:
    """The draw entry `entry` on the current stream of `out`'s device (a new int32 [n][4] on `device` when `out` is None)."""
    dev = torch.device(device) if out is None else out.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((n, 4), dtype=torch.int32, device=dev)
        _lib.check(getattr(_lib.load(), entry)(_u64(seed), _u64(step), global_batch, first, n, *scalars, out.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), entry)
    return out


def aug_draw(seed: int, step: int, global_batch: int, first: int, n: int, pad: int, flip: bool, device="cuda",
             out: torch.Tensor = None) -> torch.Tensor:
    """vdqn_aug_draw on the current stream -> int32 [n][4] {sx, sy, flip, 0} of samples first .. first + n of the global batch."""
    return _draw("vdqn_aug_draw", seed, step, global_batch, first, n, (pad, int(bool(flip))), device, out)


def aug_draw_color(seed: int, step: int, global_batch: int, first: int, n: int, jb: int, jc: int, js: int, device="cuda",
                   out: torch.Tensor = None) -> torch.Tensor:
    """vdqn_aug_draw_color on the current stream -> int32 [n][4] {f_b, f_c, f_s, 0} (Q8, 256 = 1.0) of samples first .. first + n of
    the global batch; jb, jc, js are the Q8 half-widths (`jq`)."""
    return _draw("vdqn_aug_draw_color", seed, step, global_batch, first, n, (jb, jc, js), device, out)


def aug_draw_zoom(seed: int, step: int, global_batch: int, first: int, n: int, jz: int, aspect: bool, device="cuda",
                  out: torch.Tensor = None) -> torch.Tensor:
    """vdqn_aug_draw_zoom on the current stream -> int32 [n][4] {ax, ay, bx, by} (Q16, 65536 = 1.0) of samples first .. first + n of
    the global batch; jz is the Q16 width (`jz`)."""
    return _draw("vdqn_aug_draw_zoom", seed, step, global_batch, first, n, (jz, int(bool(aspect))), device, out)


def aug_draw_rotate(seed: int, step: int, global_batch: int, first: int, n: int, jr: int, zoom: torch.Tensor = None, device="cuda",
                    out: torch.Tensor = None) -> torch.Tensor:
    """vdqn_aug_draw_rotate on the current stream -> int32 [n][8] {axx, axy, bx, 0, ayx, ayy, by, 0} (Q16) of samples first .. first + n of
    the global batch: a rotation by an angle from [-jr, jr] / 64 degrees (`jr`) composed with `zoom`, the slice's int32 [n][4] zoom rows
    (None: the identity)."""
    dev = torch.device(device) if out is None and zoom is None else (zoom if out is None else out).device
    if zoom is not None and (zoom.dtype != torch.int32 or not zoom.is_contiguous() or tuple(zoom.shape) != (n, 4) or zoom.device != dev):
        raise _lib.VdqnError(f"aug_draw_rotate: zoom must be a contiguous int32 [{n}][4] tensor on {dev}")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((n, 8), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().vdqn_aug_draw_rotate(_u64(seed), _u64(step), global_batch, first, n, jr, None if zoom is None else zoom.data_ptr(),
                                                    out.data_ptr(), torch.cuda.current_stream().cuda_stream), "vdqn_aug_draw_rotate")
    return out


def _check_rows(name: str, rows: torch.Tensor, params: torch.Tensor, words: int = 4) -> None:
    if rows is not None and (rows.dtype != torch.int32 or not rows.is_contiguous() or rows.numel() * 4 != params.numel() * words
                             or rows.device != params.device):
        raise _lib.VdqnError(f"pack_input_aug: {name} must be contiguous int32 [*][{words}] with as many rows as params, on their device")


def pack_input_aug(src: torch.Tensor, params: torch.Tensor, frames_per_sample: int, dtype: torch.dtype,
                   color: torch.Tensor = None, zoom: torch.Tensor = None, affine: torch.Tensor = None) -> torch.Tensor:
    """uint8 NHWC [n][224][224][3] frames + int32 [*][4] params (+ int32 [*][4] colour factors and / or zoom rows, or int32 [*][8] affine
    rows, each as many rows as params) -> the augmented stem operand [n][115][115][16]."""
    if src.dtype != torch.uint8 or not src.is_contiguous() or params.dtype != torch.int32 or not params.is_contiguous():
        raise _lib.VdqnError("pack_input_aug: src must be contiguous uint8 NHWC frames and params contiguous int32 [*][4]")
    _check_rows("color", color, params)
    _check_rows("zoom", zoom, params)
    _check_rows("affine", affine, params, 8)
    if zoom is not None and affine is not None:
        raise _lib.VdqnError("pack_input_aug: zoom and affine are both given, but the affine rows already contain the zoom (aug_draw_rotate "
                             "composes them): pass affine alone")
    # the entry that takes the arrays given, and those arrays behind params in its argument order (the zoom and affine entries: colour
    # may be NULL)
    if affine is not None:
        entry, rows = "vdqn_pack_input_aug_affine", (None if color is None else color.data_ptr(), affine.data_ptr())
    elif zoom is not None:
        entry, rows = "vdqn_pack_input_aug_zoom", (None if color is None else color.data_ptr(), zoom.data_ptr())
    elif color is not None:
        entry, rows = "vdqn_pack_input_aug_color", (color.data_ptr(),)
    else:
        entry, rows = "vdqn_pack_input_aug", ()
    n_img = src.numel() // (224 * 224 * 3)
    with torch.cuda.device(src.device):
        dst = torch.empty((n_img, 115, 115, 16), dtype=dtype, device=src.device)
        code = _lib.VDQN_BF16 if dtype == torch.bfloat16 else _lib.VDQN_F32
        _lib.check(getattr(_lib.load(), entry)(src.data_ptr(), dst.data_ptr(), n_img, frames_per_sample, params.data_ptr(), *rows,
                                               params.numel() // 4, code, torch.cuda.current_stream().cuda_stream), entry)
    return dst


class Augmenter:
    """The per-update draw of one rank: ``draw(step)`` -> this rank's int32 [B][4] on the device (valid until the next call),
    ``actions(act)`` -> the action labels with ``flip_actions`` exchanged for the mirrored samples of that draw.  With a colour
    half-width above 0, ``draw`` also fills ``color`` (int32 [B][4] {f_b, f_c, f_s, 0}; None when all three are 0), and with ``zoom``
    above 0 ``zoom`` (int32 [B][4] {ax, ay, bx, by}; None when off), and with ``rotate`` above 0 ``affine`` (int32 [B][8], the rotation composed
    with that zoom row; None when off: an update then takes ``affine`` and not ``zoom``)."""

    def __init__(self, batch: int, device, pad: int = 0, flip: bool = False, flip_actions=(1, 2), seed: int = 0, rank: int = 0,
                 world_size: int = 1, brightness: float = 0.0, contrast: float = 0.0, saturation: float = 0.0,
                 zoom: float = 0.0, zoom_aspect: bool = False, rotate: float = 0.0):
        check_config(pad, flip, flip_actions, brightness, contrast, saturation, zoom, zoom_aspect, rotate)
        self.lib = _lib.load()
        self.B, self.rank, self.world = int(batch), int(rank), int(world_size)
        self.G = self.B * self.world
        self.pad, self.flip, self.flip_actions, self.seed = int(pad), bool(flip), tuple(int(a) for a in flip_actions), int(seed)
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.params = torch.zeros((self.B, 4), dtype=torch.int32, device=self.device)
            self._act = torch.zeros(self.B, dtype=torch.int64, device=self.device)
            self.jq = (jq(brightness), jq(contrast), jq(saturation))
            self.color = torch.empty((self.B, 4), dtype=torch.int32, device=self.device) if any(self.jq) else None
            self.jz, self.zoom_aspect = jz(zoom), bool(zoom_aspect)
            self.zoom = torch.empty((self.B, 4), dtype=torch.int32, device=self.device) if self.jz else None
            self.jr = jr(rotate)
            self.affine = torch.empty((self.B, 8), dtype=torch.int32, device=self.device) if self.jr else None
        self.last_step = None  # the update number of the draw `params` (and `color`, `zoom`, `affine`) hold

    def draw(self, step: int) -> torch.Tensor:
        # (colour, zoom or rotation alone: `params` stays the zeros vdqn_aug_draw gives for pad 0)
        if self.pad > 0 or self.flip or (self.color is None and self.zoom is None and self.affine is None):
            aug_draw(self.seed, step, self.G, self.rank * self.B, self.B, self.pad, self.flip, out=self.params)
        if self.color is not None:
            aug_draw_color(self.seed, step, self.G, self.rank * self.B, self.B, *self.jq, out=self.color)
        if self.zoom is not None:
            aug_draw_zoom(self.seed, step, self.G, self.rank * self.B, self.B, self.jz, self.zoom_aspect, out=self.zoom)
        if self.affine is not None:  # behind the zoom draw on the same stream: it reads this update's zoom rows
            aug_draw_rotate(self.seed, step, self.G, self.rank * self.B, self.B, self.jr, zoom=self.zoom, out=self.affine)
        self.last_step = int(step)
        return self.params

    def actions(self, act: torch.Tensor) -> torch.Tensor:
        if not self.flip:
            return act
        if act.dtype != torch.int64 or act.numel() != self.B or not act.is_contiguous() or act.device != self.params.device:
            raise _lib.VdqnError(f"Augmenter.actions: act must be a contiguous int64 [{self.B}] tensor on {self.params.device}")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vdqn_aug_swap_actions(act.data_ptr(), self.params.data_ptr(), self.B, self.flip_actions[0], self.flip_actions[1],
                                                      self._act.data_ptr(), torch.cuda.current_stream().cuda_stream), "vdqn_aug_swap_actions")
        return self._act
