"""Host-side mirror of reference `imagekit::transform` (src/transform.rs).

The same three functions with the same argument meaning and error behaviour:

    decode_image(bytes) -> (DynamicImage, Optional[ImageFormat])       :27-43
    resize_image(img, w: Optional[int], h: Optional[int]) -> DynamicImage  :62-90
    encode_image(img, fmt: ImageFormat, quality: int) -> bytes          :113-150

Every call goes through libimagekit_hip.so (include/imagekit_hip.h): pixels live
in HBM as a device-resident `DynamicImage`; the resampler, the colour
conversions and the FDCT/quantiser are gfx950 kernels.  Failures raise
`TransformError`, as the reference maps every decode/encode failure to
`ImageKitError::TransformError`.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import enum
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .config import ImageFormat
from .errors import InvalidArgument, TransformError


class FilterType(enum.IntEnum):
    """image::imageops::FilterType (image 0.25.8).  resize_image uses Lanczos3."""

    Nearest = 0
    Triangle = 1
    CatmullRom = 2
    Gaussian = 3
    Lanczos3 = 4


class FitMode(enum.IntEnum):
    """ik_fit: how a request's (w, h) becomes pixels (the reference's query parser
    declares fit=cover|contain, src/transform/params.rs:37-64).  contain is
    DynamicImage::resize (resize_image as the reference calls it), cover
    DynamicImage::resize_to_fill, exact DynamicImage::resize_exact."""

    contain = 0
    cover = 1
    exact = 2


def _fits(fits, n):
    """The per-request fit array of a batch call, or None (every request contain)."""
    if fits is None:
        return None
    if len(fits) != n:
        raise InvalidArgument("fits must have one entry per request")
    return (ctypes.c_int * n)(*[int(FitMode(f)) for f in fits])


class Orientation(enum.IntEnum):
    """ik_orient / image::metadata::Orientation by its EXIF value: what the `orient=`
    arguments take.  stored (the default everywhere) leaves the pixels as the file holds
    them, as the reference's decode_image does; auto applies the file's EXIF Orientation
    (exif_orientation); the eight values apply that one whatever the file says."""

    auto = -1
    stored = 0
    no_transforms = 1
    flip_horizontal = 2
    rotate180 = 3
    flip_vertical = 4
    rotate90_flip_h = 5
    rotate90 = 6
    rotate270_flip_h = 7
    rotate270 = 8


def _orient(o) -> int:
    try:
        return int(Orientation(o))
    except ValueError:
        raise InvalidArgument(f"unknown orientation {o!r}") from None


def _orients(orients, n):
    """The per-request orientation array of a batch call, or None (every request stored)."""
    if orients is None:
        return None
    if len(orients) != n:
        raise InvalidArgument("orients must have one entry per request")
    return (ctypes.c_int * n)(*[_orient(o) for o in orients])


BG_NONE = -1  # IK_BG_NONE


def _background(bg) -> int:
    """A `background=` argument as ik_request_opts.background: None (no flatten: IK_BG_NONE),
    an int 0xRRGGBB, an (r, g, b) tuple of 0..255, or an "rrggbb" / "#rrggbb" string.
    Anything else raises ValueError, before the library is called."""
    if bg is None:
        return BG_NONE
    if isinstance(bg, bool):
        raise ValueError(f"background {bg!r} is not a colour")
    if isinstance(bg, (int, np.integer)):
        if not 0 <= int(bg) <= 0xFFFFFF:
            raise ValueError(f"background {bg!r} outside 0x000000..0xFFFFFF")
        return int(bg)
    if isinstance(bg, str):
        s = bg[1:] if bg.startswith("#") else bg
        if len(s) != 6 or any(ch not in "0123456789abcdefABCDEF" for ch in s):
            raise ValueError(f"background {bg!r} is not rrggbb")
        return int(s, 16)
    if isinstance(bg, (tuple, list)):
        if len(bg) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255
                               for v in bg):
            raise ValueError(f"background {bg!r} is not (r, g, b) of 0..255")
        return (int(bg[0]) << 16) | (int(bg[1]) << 8) | int(bg[2])
    raise ValueError(f"background {bg!r} is not a colour")


BLUR_MIN_SIGMA, BLUR_MAX_SIGMA = 0.0625, 32.0  # IK_BLUR_MAX_SIGMA


def _sigma(v, what="sigma") -> float:
    """A sigma argument: None or 0 (off: 0.0), or a number within [0.0625, 32].  Anything
    else raises ValueError, before the library is called."""
    if v is None:
        return 0.0
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} {v!r} is not a number")
    f = float(v)
    if f == 0.0:
        return 0.0
    if not BLUR_MIN_SIGMA <= f <= BLUR_MAX_SIGMA:  # (a NaN fails both comparisons)
        raise ValueError(f"{what} {v!r} outside {BLUR_MIN_SIGMA}..{BLUR_MAX_SIGMA}")
    return f


def _sharpen(v) -> Tuple[float, int]:
    """A `sharpen=` argument as (sigma, threshold): None (off), a sigma, or (sigma,
    threshold) with the threshold an int in 0..65535, in the sample's own units."""
    if v is None:
        return 0.0, 0
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"sharpen {v!r} is not (sigma, threshold)")
        t = v[1]
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) <= 65535:
            raise ValueError(f"sharpen threshold {t!r} is not an int in 0..65535")
        return _sigma(v[0], "sharpen sigma"), int(t)
    return _sigma(v, "sharpen sigma"), 0


def _filter_args(blur, sharpen) -> Tuple[float, float, int]:
    """(blur sigma, sharpen sigma, sharpen threshold) of one request; both at once is a
    ValueError, as the library refuses it."""
    b = _sigma(blur, "blur sigma")
    s, t = _sharpen(sharpen)
    if b and s:
        raise ValueError("blur and sharpen together")
    return b, s, t


class Gravity(enum.IntEnum):
    """ik_gravity: the edge or corner of the base a watermark is placed against."""

    center = 0
    n = 1
    s = 2
    e = 3
    w = 4
    ne = 5
    nw = 6
    se = 7
    sw = 8


OVERLAY_MAX_OFFSET = 1 << 24


class Overlay:
    """A watermark: an image composited over the output before it is encoded (DESIGN section
    4).  image: the mark, a DynamicImage prepared once (it is never resized or turned here)
    and shared by any number of requests; gravity: a Gravity or its name; dx, dy: signed
    pixel offsets added to the gravity's origin; opacity 1..255; tile: repeat the mark over
    the whole image.  Anything else raises ValueError, before the library is called."""

    __slots__ = ("image", "gravity", "dx", "dy", "opacity", "tile")

    def __init__(self, image: "DynamicImage", gravity=Gravity.center, dx: int = 0, dy: int = 0, opacity: int = 255,
                 tile: bool = False):
        if not isinstance(image, DynamicImage):
            raise ValueError(f"overlay image {image!r} is not a DynamicImage")
        try:
            self.gravity = Gravity[gravity.lower()] if isinstance(gravity, str) else Gravity(gravity)
        except (KeyError, ValueError):
            raise ValueError(f"unknown gravity {gravity!r}") from None
        for name, v in (("dx", dx), ("dy", dy)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or abs(int(v)) > OVERLAY_MAX_OFFSET:
                raise ValueError(f"overlay {name} {v!r} is not an int within +-{OVERLAY_MAX_OFFSET}")
        if isinstance(opacity, bool) or not isinstance(opacity, (int, np.integer)) or not 1 <= int(opacity) <= 255:
            raise ValueError(f"overlay opacity {opacity!r} is not an int in 1..255")
        if not isinstance(tile, (bool, np.bool_)):
            raise ValueError(f"overlay tile {tile!r} is not a bool")
        self.image, self.dx, self.dy, self.opacity, self.tile = image, int(dx), int(dy), int(opacity), bool(tile)

    def _fill(self, ro) -> None:
        """this watermark into an ik_request_opts3"""
        ro.overlay = self.image._h.value
        ro.overlay_gravity, ro.overlay_dx, ro.overlay_dy = int(self.gravity), self.dx, self.dy
        ro.overlay_opacity, ro.overlay_tile, ro.reserved = self.opacity, int(self.tile), 0


def _overlay(v) -> Optional[Overlay]:
    """An `overlay=` argument: None, an Overlay, or a DynamicImage (an opaque centred mark)."""
    if v is None or isinstance(v, Overlay):
        return v
    return Overlay(v)


def _overlays(overlays, n) -> Optional[list]:
    """The per-request watermarks of a batch call, or None (no request has one): one entry per
    request, or a single Overlay / DynamicImage (or a list of one) that applies to all."""
    if overlays is None:
        return None
    if isinstance(overlays, (Overlay, DynamicImage)):
        overlays = [overlays]
    if len(overlays) == 1 and n != 1:
        overlays = list(overlays) * n
    if len(overlays) != n:
        raise InvalidArgument("overlays must have one entry per request, or one for all")
    marks = [_overlay(v) for v in overlays]
    return marks if any(m is not None for m in marks) else None


class Adjust:
    """A colour adjustment of the output's pixels (ik_adjust): brightness,
    contrast and saturation are ints in -100..100 (0: none; saturation -100 is grayscale),
    hue degrees in -360..360, gamma None or 0 (none) or a number within 0.1..10, invert a
    bool; grayscale=True is sugar for saturation -100.  Alpha is never touched.  Anything
    else raises ValueError, before the library is called."""

    __slots__ = ("brightness", "contrast", "saturation", "hue", "gamma", "invert")

    def __init__(self, brightness: int = 0, contrast: int = 0, saturation: int = 0, hue: int = 0, gamma=None,
                 invert: bool = False, grayscale: bool = False):
        if not isinstance(grayscale, (bool, np.bool_)):
            raise ValueError(f"adjust grayscale {grayscale!r} is not a bool")
        if grayscale:
            if saturation not in (0, -100):
                raise ValueError("grayscale and a saturation together")
            saturation = -100
        for name, v, lim in (("brightness", brightness, 100), ("contrast", contrast, 100),
                             ("saturation", saturation, 100), ("hue", hue, 360)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or abs(int(v)) > lim:
                raise ValueError(f"adjust {name} {v!r} is not an int within +-{lim}")
        if gamma is None:
            gamma = 0.0
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)):
            raise ValueError(f"adjust gamma {gamma!r} is not a number")
        g = float(np.float32(gamma))
        if g != 0.0 and not float(np.float32(0.1)) <= g <= 10.0:  # (a NaN fails both comparisons)
            raise ValueError(f"adjust gamma {gamma!r} is neither 0 nor within 0.1..10")
        if not isinstance(invert, (bool, np.bool_)):
            raise ValueError(f"adjust invert {invert!r} is not a bool")
        self.brightness, self.contrast, self.saturation, self.hue = int(brightness), int(contrast), int(saturation), int(hue)
        self.gamma, self.invert = g, bool(invert)

    def is_none(self) -> bool:
        return not (self.brightness or self.contrast or self.saturation or self.hue or self.gamma or self.invert)

    def _struct(self) -> "_lib.Adjust":
        return _lib.Adjust(self.brightness, self.contrast, self.saturation, self.hue, self.gamma, int(self.invert))


def _adjust(v) -> Optional[Adjust]:
    """An `adjust=` argument: None, an Adjust, or a dict of Adjust's keyword arguments.  One
    that changes nothing is None."""
    if v is None:
        return None
    if isinstance(v, dict):
        v = Adjust(**v)
    if not isinstance(v, Adjust):
        raise ValueError(f"adjust {v!r} is not an Adjust")
    return None if v.is_none() else v


def _adjusts(adjusts, n) -> Optional[list]:
    """The per-request adjustments of a batch call, or None (no request has one): one entry
    per request, or a single Adjust (or a list of one) that applies to all."""
    if adjusts is None:
        return None
    if isinstance(adjusts, (Adjust, dict)):
        adjusts = [adjusts]
    if len(adjusts) == 1 and n != 1:
        adjusts = list(adjusts) * n
    if len(adjusts) != n:
        raise InvalidArgument("adjusts must have one entry per request, or one for all")
    adj = [_adjust(v) for v in adjusts]
    return adj if any(a is not None for a in adj) else None


class PadMode(enum.IntEnum):
    """ik_pad_mode: what the frame of a pad is made of."""
    color = 1
    edge = 2
    mirror = 3
    wrap = 4


class Pad:
    """The output extended onto a canvas (ik_pad): mode a PadMode or its name
    ("color", "edge", "mirror", "wrap"), gravity a Gravity or its name (where the image lies in
    the canvas), width and height ints in 0..2**24 (0: the side of the request's box in a
    transform call, the image's own side in DynamicImage.pad), color as `background` takes it
    (0xRRGGBB, (r, g, b), "rrggbb" or "#rrggbb"), alpha 0..255: the frame's alpha where the
    image has one.  Anything else raises ValueError, before the library is called."""

    __slots__ = ("mode", "gravity", "width", "height", "color", "alpha")

    def __init__(self, mode="color", gravity="center", width: int = 0, height: int = 0, color=0, alpha: int = 255):
        try:
            self.mode = PadMode[mode.lower()] if isinstance(mode, str) else PadMode(mode)
        except (KeyError, ValueError):
            raise ValueError(f"unknown pad mode {mode!r}") from None
        try:
            self.gravity = Gravity[gravity.lower()] if isinstance(gravity, str) else Gravity(gravity)
        except (KeyError, ValueError):
            raise ValueError(f"unknown pad gravity {gravity!r}") from None
        for name, v in (("width", width), ("height", height)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 1 << 24:
                raise ValueError(f"pad {name} {v!r} is not an int within 0..2**24")
        if isinstance(alpha, bool) or not isinstance(alpha, (int, np.integer)) or not 0 <= int(alpha) <= 255:
            raise ValueError(f"pad alpha {alpha!r} is not an int within 0..255")
        c = _background(color)
        if c == BG_NONE:
            raise ValueError("pad color None")
        self.width, self.height, self.color, self.alpha = int(width), int(height), c, int(alpha)

    def _struct(self) -> "_lib.Pad":
        return _lib.Pad(int(self.mode), int(self.gravity), self.width, self.height, self.color, self.alpha)


def _pad(v) -> Optional[Pad]:
    """A `pad=` argument: None, a Pad, or a dict of Pad's keyword arguments."""
    if v is None:
        return None
    if isinstance(v, dict):
        v = Pad(**v)
    if not isinstance(v, Pad):
        raise ValueError(f"pad {v!r} is not a Pad")
    return v


def _pads(pads, n) -> Optional[list]:
    """The per-request pads of a batch call, or None (no request has one): one entry per
    request, or a single Pad (or a list of one) that applies to all."""
    if pads is None:
        return None
    if isinstance(pads, (Pad, dict)):
        pads = [pads]
    if len(pads) == 1 and n != 1:
        pads = list(pads) * n
    if len(pads) != n:
        raise InvalidArgument("pads must have one entry per request, or one for all")
    pd = [_pad(v) for v in pads]
    return pd if any(p is not None for p in pd) else None


def _request_opts(n, fits=None, orients=None, backgrounds=None, blurs=None, sharpens=None, overlays=None,
                  adjusts=None, pads=None):
    """The options array of a *_opts batch call (each argument: one entry per request, or
    None for that option's default everywhere): ik_request_opts, ik_request_opts2 when
    blurs or sharpens is given, ik_request_opts3 when some request has an overlay,
    ik_request_opts4 when some request has an adjustment, or ik_request_opts5 when some
    request pads.  Its element size is
    ctypes.sizeof(arr._type_).  The overlays' images must outlive the call (a submitted
    batch: its wait)."""
    for name, v in (("fits", fits), ("orient", orients), ("backgrounds", backgrounds), ("blurs", blurs),
                    ("sharpens", sharpens)):
        if v is not None and len(v) != n:
            raise InvalidArgument(f"{name} must have one entry per request")
    marks = _overlays(overlays, n)
    adj = _adjusts(adjusts, n)
    pd = _pads(pads, n)
    wide = blurs is not None or sharpens is not None or marks is not None or adj is not None or pd is not None
    arr = ((_lib.RequestOpts5 if pd is not None else _lib.RequestOpts4 if adj is not None
            else _lib.RequestOpts3 if marks is not None else _lib.RequestOpts2 if wide else _lib.RequestOpts) * n)()
    for i in range(n if pd is not None else 0):
        if pd[i] is not None:
            arr[i].pad = pd[i]._struct()
    for i in range(n if adj is not None else 0):
        if adj[i] is not None:
            arr[i].adjust = adj[i]._struct()
    for i in range(n if wide else 0):
        arr[i].blur_sigma, arr[i].sharpen_sigma, arr[i].sharpen_threshold = _filter_args(
            blurs[i] if blurs is not None else None, sharpens[i] if sharpens is not None else None)
    for i in range(n if marks is not None else 0):
        if marks[i] is not None:
            marks[i]._fill(arr[i])
    for i in range(n):
        arr[i].fit = int(FitMode(fits[i])) if fits is not None else int(FitMode.contain)
        arr[i].orient = _orient(orients[i]) if orients is not None else int(Orientation.stored)
        arr[i].background = _background(backgrounds[i]) if backgrounds is not None else BG_NONE
    return arr


def exif_orientation(data: bytes) -> int:
    """ImageDecoder::orientation() as its EXIF value, 1..8: JPEG APP1, PNG eXIf, WebP EXIF;
    1 when the file carries none or it cannot be read (ik_exif_orientation; host only)."""
    b = bytes(data)
    return int(_lib.load().ik_exif_orientation(b, len(b)))


_COLOR = {1: "L8", 2: "La8", 3: "Rgb8", 4: "Rgba8"}


def _raise(status: int, what: str):
    msg = _lib.last_error()
    if status == 2:
        raise InvalidArgument(f"{what}: {msg}")
    raise TransformError(msg)


class DynamicImage:
    """An 8-bit image (L8 / La8 / Rgb8 / Rgba8) resident in device memory."""

    __slots__ = ("_h", "__weakref__")

    def __init__(self, handle: int):
        self._h = ctypes.c_void_p(handle)

    @classmethod
    def from_array(cls, pixels: np.ndarray) -> "DynamicImage":
        """ImageBuffer::from_raw on an (H, W) or (H, W, C) array: uint8 (L8 / La8 /
        Rgb8 / Rgba8) or uint16 (L16 / La16 / Rgb16 / Rgba16)."""
        wide = np.asarray(pixels).dtype == np.uint16
        a = np.ascontiguousarray(pixels, dtype=np.uint16 if wide else np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3 or not 1 <= a.shape[2] <= 4:
            raise InvalidArgument("expected (H, W, C) uint8 or uint16 with C in 1..4")
        h, w, c = a.shape
        lib = _lib.load()
        out = ctypes.c_void_p()
        st = (lib.ik_image_from_host16 if wide else lib.ik_image_from_host)(a.ctypes.data, w, h, c, ctypes.byref(out))
        if st:
            _raise(st, "from_array")
        return cls(out.value)

    @classmethod
    def new_rgb8(cls, w: int, h: int) -> "DynamicImage":
        """DynamicImage::new_rgb8 (all-zero pixels), as tests/transform.rs builds inputs."""
        return cls.from_array(np.zeros((h, w, 3), np.uint8))

    @classmethod
    def new_rgba8(cls, w: int, h: int) -> "DynamicImage":
        return cls.from_array(np.zeros((h, w, 4), np.uint8))

    def dimensions(self) -> Tuple[int, int]:
        w, h, c = self._info()
        return (w, h)

    def width(self) -> int:
        return self._info()[0]

    def height(self) -> int:
        return self._info()[1]

    @property
    def channels(self) -> int:
        return self._info()[2]

    def color(self) -> str:
        name = _COLOR[self._info()[2]]
        return name.replace("8", "16") if self.depth == 2 else name

    def _info(self):
        lib = _lib.load()
        w, h, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        st = lib.ik_image_info(self._h, ctypes.byref(w), ctypes.byref(h), ctypes.byref(c))
        if st:
            _raise(st, "image_info")
        return w.value, h.value, c.value

    @property
    def depth(self) -> int:
        """Bytes per sample: 1 (8-bit) or 2 (16-bit)."""
        return int(_lib.load().ik_image_depth(self._h))

    def to_array(self) -> np.ndarray:
        """Copy the pixels back to the host as an (H, W, C) array (uint8, or uint16
        for a 16-bit image)."""
        w, h, c = self._info()
        out = np.empty((h, w, c), np.uint16 if self.depth == 2 else np.uint8)
        st = _lib.load().ik_image_to_host(self._h, out.ctypes.data, out.nbytes)
        if st:
            _raise(st, "to_array")
        return out

    def resize(self, nw: int, nh: int, filter: FilterType = FilterType.Lanczos3) -> "DynamicImage":
        """imageops::resize to exactly nw x nh (the resampler under resize_image)."""
        out = ctypes.c_void_p()
        st = _lib.load().ik_resize_exact(self._h, nw, nh, int(filter), ctypes.byref(out))
        if st:
            _raise(st, "resize")
        return DynamicImage(out.value)

    def resize_exact(self, nw: int, nh: int, filter: FilterType = FilterType.Lanczos3) -> "DynamicImage":
        """DynamicImage::resize_exact: nw x nh, the aspect ratio not kept."""
        return self.resize(nw, nh, filter)

    def resize_to_fill(self, nw: int, nh: int, filter: FilterType = FilterType.Lanczos3) -> "DynamicImage":
        """DynamicImage::resize_to_fill: scaled to cover nw x nh, then cropped to it about
        the centre (only the kept window is computed)."""
        return resize_image(self, nw, nh, filter, fit=FitMode.cover)

    def apply_orientation(self, o) -> "DynamicImage":
        """DynamicImage::apply_orientation as a new image (ik_image_orient): o is an EXIF
        value 1..8 (Orientation); 1 copies."""
        o = _orient(o)
        if not 1 <= o <= 8:
            raise InvalidArgument("apply_orientation takes an EXIF value 1..8")
        out = ctypes.c_void_p()
        st = _lib.load().ik_image_orient(self._h, o, ctypes.byref(out))
        if st:
            _raise(st, "apply_orientation")
        return DynamicImage(out.value)

    def flatten(self, background) -> "DynamicImage":
        """The image composited onto a background colour as a new image (ik_image_flatten;
        the project's own arithmetic): Rgba -> Rgb, LumaA -> Luma for a gray
        colour and Rgb for any other; an image without alpha, or None, gives a copy."""
        out = ctypes.c_void_p()
        st = _lib.load().ik_image_flatten(self._h, _background(background), ctypes.byref(out))
        if st:
            _raise(st, "flatten")
        return DynamicImage(out.value)

    def blur(self, sigma: float) -> "DynamicImage":
        """A Gaussian blur of the image as a new image (ik_image_blur; the project's own
        definition): sigma within [0.0625, 32], channels and depth kept."""
        f = _sigma(sigma)
        if not f:
            raise ValueError(f"sigma {sigma!r} outside {BLUR_MIN_SIGMA}..{BLUR_MAX_SIGMA}")
        out = ctypes.c_void_p()
        st = _lib.load().ik_image_blur(self._h, f, ctypes.byref(out))
        if st:
            _raise(st, "blur")
        return DynamicImage(out.value)

    def unsharpen(self, sigma: float, threshold: int = 0) -> "DynamicImage":
        """The unsharp mask as a new image (ik_image_unsharpen): with B the blur of sigma,
        a sample S whose |S - B| exceeds threshold becomes clamp(2 S - B)."""
        f, t = _sharpen((sigma, threshold))
        if not f:
            raise ValueError(f"sigma {sigma!r} outside {BLUR_MIN_SIGMA}..{BLUR_MAX_SIGMA}")
        out = ctypes.c_void_p()
        st = _lib.load().ik_image_unsharpen(self._h, f, t, ctypes.byref(out))
        if st:
            _raise(st, "unsharpen")
        return DynamicImage(out.value)

    def overlay(self, mark, gravity=Gravity.center, dx: int = 0, dy: int = 0, opacity: int = 255,
                tile: bool = False) -> "DynamicImage":
        """This image under a watermark as a new image (ik_image_overlay; the project's own
        definition): mark is a DynamicImage (or an Overlay, which carries the
        other arguments itself); channels and depth are this image's."""
        o = mark if isinstance(mark, Overlay) else Overlay(mark, gravity, dx, dy, opacity, tile)
        out = ctypes.c_void_p()
        st = _lib.load().ik_image_overlay(self._h, o.image._h, int(o.gravity), o.dx, o.dy, o.opacity, int(o.tile),
                                          ctypes.byref(out))
        if st:
            _raise(st, "overlay")
        return DynamicImage(out.value)

    def adjust(self, adjust=None, **kwargs) -> "DynamicImage":
        """This image under a colour adjustment as a new image (ik_image_adjust; the project's
        own definition): an Adjust, or Adjust's keyword arguments
        (img.adjust(grayscale=True)); channels and depth are kept, alpha is not touched."""
        if adjust is not None and kwargs:
            raise ValueError("an Adjust and keyword arguments together")
        a = adjust if adjust is not None else Adjust(**kwargs)
        if isinstance(a, dict):
            a = Adjust(**a)
        if not isinstance(a, Adjust):
            raise ValueError(f"adjust {a!r} is not an Adjust")
        st_a = a._struct()
        out = ctypes.c_void_p()
        st = _lib.load().ik_image_adjust(self._h, ctypes.byref(st_a), ctypes.byref(out))
        if st:
            _raise(st, "adjust")
        return DynamicImage(out.value)

    def pad(self, pad=None, **kwargs) -> "DynamicImage":
        """This image on a canvas as a new image (ik_image_pad; the project's own definition,
        DESIGN section 4): a Pad, or Pad's keyword arguments (img.pad(width=512, height=512,
        color="ffffff")); a width or height of 0, or one the image already fills, leaves that
        axis alone.  Channels and depth are kept."""
        if pad is not None and kwargs:
            raise ValueError("a Pad and keyword arguments together")
        p = pad if pad is not None else Pad(**kwargs)
        if isinstance(p, dict):
            p = Pad(**p)
        if not isinstance(p, Pad):
            raise ValueError(f"pad {p!r} is not a Pad")
        st_p = p._struct()
        out = ctypes.c_void_p()
        st = _lib.load().ik_image_pad(self._h, ctypes.byref(st_p), ctypes.byref(out))
        if st:
            _raise(st, "pad")
        return DynamicImage(out.value)

    def clone(self) -> "DynamicImage":
        return DynamicImage.from_array(self.to_array())

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib._lib is not None:
            _lib._lib.ik_image_free(h)
            self._h = ctypes.c_void_p(0)

    def __repr__(self) -> str:
        w, h, c = self._info()
        return f"DynamicImage({_COLOR[c]}, {w}x{h}, device)"


def decode_image(data: bytes, orient=Orientation.stored) -> Tuple[DynamicImage, Optional[ImageFormat]]:
    """src/transform.rs:27-43 -- guess_format + load_from_memory_with_format.  orient (an
    extension: Orientation) turns the decoded image; the default leaves it as stored."""
    lib = _lib.load()
    b = bytes(data)
    out = ctypes.c_void_p()
    fmt = ctypes.c_int(-1)
    o = _orient(orient)
    if o == Orientation.stored:
        st = lib.ik_decode(b, len(b), ctypes.byref(out), ctypes.byref(fmt))
    else:
        st = lib.ik_decode_oriented(b, len(b), o, ctypes.byref(out), ctypes.byref(fmt))
    if st:
        raise TransformError(_lib.last_error())
    f = None if fmt.value < 0 else ImageFormat(fmt.value)
    return DynamicImage(out.value), f


def decode_image_batch(datas) -> List[Tuple[DynamicImage, Optional[ImageFormat]]]:
    """decode_image over many inputs with one GPU entropy-decoding launch for the
    restart-interval JPEGs among them (ik_decode_batch).  Raises the first failure."""
    lib = _lib.load()
    bufs = [bytes(d) for d in datas]
    n = len(bufs)
    if n == 0:
        return []
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
    lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
    outs = (ctypes.c_void_p * n)()
    fmts = (ctypes.c_int * n)()
    status = (ctypes.c_int * n)()
    st = lib.ik_decode_batch(ptrs, lens, n, outs, fmts, status)
    imgs = [DynamicImage(outs[i]) if outs[i] else None for i in range(n)]
    if st:
        raise TransformError(_lib.last_error())
    return [(imgs[i], None if fmts[i] < 0 else ImageFormat(fmts[i])) for i in range(n)]


class PinnedBytes:
    """Encoded input bytes in page-locked host memory (ik_host_alloc): the batch
    calls DMA them to the GPU in place, with no staging copy -- what a server does
    by reading request bodies into such buffers.  Accepted wherever the batch
    calls take `bytes`."""

    __slots__ = ("ptr", "len", "__weakref__")

    def __init__(self, data: bytes):
        lib = _lib.load()
        p = ctypes.c_void_p()
        if lib.ik_host_alloc(max(1, len(data)), ctypes.byref(p)) != 0:
            raise TransformError(_lib.last_error())
        ctypes.memmove(p, data, len(data))
        self.ptr, self.len = p.value, len(data)

    def __len__(self) -> int:
        return self.len

    def tobytes(self) -> bytes:
        return ctypes.string_at(self.ptr, self.len)

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                _lib.load().ik_host_free(ctypes.c_void_p(self.ptr))
            except Exception:
                pass
            self.ptr = None


class DeviceBytes:
    """Encoded input bytes in device memory (ik_dev_alloc on the current device):
    request bodies a caller already holds in HBM, for transform_batch_submit_device."""

    __slots__ = ("ptr", "len", "__weakref__")

    def __init__(self, data: bytes):
        lib = _lib.load()
        p = ctypes.c_void_p()
        if lib.ik_dev_alloc(max(1, len(data)), ctypes.byref(p)) != 0:
            raise TransformError(_lib.last_error())
        if len(data) and lib.ik_memcpy_h2d(p, bytes(data), len(data)) != 0:
            lib.ik_dev_free(p)
            raise TransformError(_lib.last_error())
        self.ptr, self.len = p.value, len(data)

    def __len__(self) -> int:
        return self.len

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                _lib.load().ik_dev_free(ctypes.c_void_p(self.ptr))
            except Exception:
                pass
            self.ptr = None


def _inputs(datas):
    """(keep-alive list, pointer array, length array) for a batch call."""
    keep = [d if isinstance(d, PinnedBytes) else bytes(d) for d in datas]
    n = len(keep)
    ptrs = (ctypes.c_void_p * n)(*[d.ptr if isinstance(d, PinnedBytes) else
                                   ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p).value for d in keep])
    lens = (ctypes.c_size_t * n)(*[len(d) for d in keep])
    return keep, ptrs, lens


def _batch_arrays(n, sizes, fmts, qualities, filter):
    """What every batch call passes beside its inputs and options: the (w, h), format and
    quality arrays, the filter, and the output, length and status arrays the library fills."""
    filt = int(FilterType.Lanczos3 if filter is None else filter)
    ws = (ctypes.c_int64 * n)(*[-1 if s[0] is None else int(s[0]) for s in sizes])
    hs = (ctypes.c_int64 * n)(*[-1 if s[1] is None else int(s[1]) for s in sizes])
    fs = (ctypes.c_int * n)(*[int(f.value if isinstance(f, ImageFormat) else f) for f in fmts])
    qs = (ctypes.c_int * n)(*[int(q) for q in qualities])
    return ws, hs, fs, qs, filt, (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()


def transform_batch(datas, sizes, fmts, qualities, filter: "FilterType" = None, threads: int = 0,
                    fits=None, orient=None, backgrounds=None, blurs=None, sharpens=None,
                    overlays=None, adjusts=None, pads=None) -> List[bytes]:
    """ik_transform_batch: decode -> resize_image -> encode_image for many requests
    (sizes: (w, h) per request, None = unset; fmts: ImageFormat per request; fits: a
    FitMode per request, None = contain for all; orient: an Orientation per request,
    None = stored for all; backgrounds: a colour per request as `transform` takes it,
    None = no flatten for any; blurs: a sigma per request, sharpens: a sigma or (sigma,
    threshold) per request, None = off; overlays: an Overlay (or a DynamicImage: an opaque
    centred mark, or None) per request, or one for all of them.  With backgrounds, blurs,
    sharpens, overlays or adjusts the call is ik_transform_batch_opts; adjusts: an Adjust (or
    None) per request, or one for all of them, applied after the resize; pads: a Pad (or
    None) per request, or one for all of them: the result placed on a canvas, a Pad size of
    0 being the side of the request's box)."""
    lib = _lib.load()
    bufs, ptrs, lens = _inputs(datas)
    n = len(bufs)
    if n == 0:
        return []
    ws, hs, fs, qs, filt, outs, olens, status = _batch_arrays(n, sizes, fmts, qualities, filter)
    fa = _fits(fits, n)
    oa = _orients(orient, n)
    if (backgrounds is not None or blurs is not None or sharpens is not None or overlays is not None
            or adjusts is not None or pads is not None):
        ra = _request_opts(n, fits, orient, backgrounds, blurs, sharpens, overlays, adjusts=adjusts, pads=pads)
        st = lib.ik_transform_batch_opts(ptrs, lens, n, ws, hs, ra, ctypes.sizeof(ra._type_), fs, qs, filt,
                                         threads, outs, olens, status)
    elif oa is not None:
        st = lib.ik_transform_batch_oriented(ptrs, lens, n, ws, hs, fa, oa, fs, qs, filt, threads, outs, olens, status)
    elif fa is None:
        st = lib.ik_transform_batch(ptrs, lens, n, ws, hs, fs, qs, filt, threads, outs, olens, status)
    else:
        st = lib.ik_transform_batch_fit(ptrs, lens, n, ws, hs, fa, fs, qs, filt, threads, outs, olens, status)
    res = []
    for i in range(n):
        res.append(ctypes.string_at(outs[i], olens[i]) if outs[i] else None)
        if outs[i]:
            lib.ik_buf_free(outs[i])
    if st:
        raise TransformError(_lib.last_error())
    return res


class PendingBatch:
    """A submitted ik_transform_batch_submit: its device half has run; wait() blocks
    until its host coders are done and returns the encoded bytes per request (the
    ctypes arrays the library writes into live here until then)."""

    def __init__(self, keep, outs, olens, status, ticket, n):
        self._keep, self._outs, self._olens, self._status = keep, outs, olens, status
        self._ticket, self._n, self._done = ticket, n, False

    def wait(self) -> List[bytes]:
        if self._done:
            raise InvalidArgument("batch already waited for")
        lib = _lib.load()
        st = lib.ik_transform_batch_wait(self._ticket)
        self._done = True
        res = []
        for i in range(self._n):
            o = self._outs[i]
            res.append(ctypes.string_at(o, self._olens[i]) if o else None)
            if o:
                lib.ik_buf_free(o)
        if st:
            raise TransformError(_lib.last_error())
        return res


def transform_batch_submit(datas, sizes, fmts, qualities, filter: "FilterType" = None,
                           threads: int = 0, fits=None, orient=None, backgrounds=None, blurs=None,
                           sharpens=None, overlays=None, adjusts=None, pads=None) -> PendingBatch:
    """ik_transform_batch_submit: the device half of transform_batch now, the host
    coders in the background; PendingBatch.wait() gives what transform_batch gives.
    fits, orient, backgrounds, blurs, sharpens and overlays as transform_batch takes them
    (the PendingBatch keeps the overlays' images alive until its wait)."""
    lib = _lib.load()
    bufs, ptrs, lens = _inputs(datas)
    n = len(bufs)
    if n == 0:
        raise InvalidArgument("empty batch")
    ws, hs, fs, qs, filt, outs, olens, status = _batch_arrays(n, sizes, fmts, qualities, filter)
    ticket = ctypes.c_uint64()
    fa = _fits(fits, n)
    oa = _orients(orient, n)
    ra = None
    if (backgrounds is not None or blurs is not None or sharpens is not None or overlays is not None
            or adjusts is not None or pads is not None):
        ra = _request_opts(n, fits, orient, backgrounds, blurs, sharpens, overlays, adjusts=adjusts, pads=pads)
        st = lib.ik_transform_batch_submit_opts(ptrs, lens, n, ws, hs, ra, ctypes.sizeof(ra._type_), fs, qs,
                                                filt, threads, outs, olens, status, ctypes.byref(ticket))
    elif oa is not None:
        st = lib.ik_transform_batch_submit_oriented(ptrs, lens, n, ws, hs, fa, oa, fs, qs, filt, threads, outs, olens,
                                                    status, ctypes.byref(ticket))
    elif fa is None:
        st = lib.ik_transform_batch_submit(ptrs, lens, n, ws, hs, fs, qs, filt, threads, outs, olens, status,
                                           ctypes.byref(ticket))
    else:
        st = lib.ik_transform_batch_submit_fit(ptrs, lens, n, ws, hs, fa, fs, qs, filt, threads, outs, olens, status,
                                               ctypes.byref(ticket))
    if st:
        raise TransformError(_lib.last_error())
    return PendingBatch((bufs, ptrs, lens, ws, hs, fs, qs, fa, oa, ra, overlays), outs, olens, status, ticket.value, n)


def transform_batch_submit_device(datas, sizes, fmts, qualities, filter: "FilterType" = None,
                                  threads: int = 0, fits=None, orient=None, backgrounds=None, blurs=None,
                                  sharpens=None, overlays=None, adjusts=None, pads=None) -> PendingBatch:
    """ik_transform_batch_submit_device: as transform_batch_submit, over request
    bodies already in device memory (DeviceBytes).  With fits, orient, backgrounds, blurs, sharpens or
    overlays the call is ik_transform_batch_submit_device_opts; Orientation.auto is refused there (the
    files are not read on the host)."""
    lib = _lib.load()
    keep = list(datas)
    n = len(keep)
    if n == 0:
        raise InvalidArgument("empty batch")
    if not all(isinstance(d, DeviceBytes) for d in keep):
        raise InvalidArgument("transform_batch_submit_device takes DeviceBytes")
    ptrs = (ctypes.c_void_p * n)(*[d.ptr for d in keep])
    lens = (ctypes.c_size_t * n)(*[len(d) for d in keep])
    ws, hs, fs, qs, filt, outs, olens, status = _batch_arrays(n, sizes, fmts, qualities, filter)
    ticket = ctypes.c_uint64()
    ra = None
    if (fits is None and orient is None and backgrounds is None and blurs is None and sharpens is None
            and overlays is None and adjusts is None and pads is None):
        st = lib.ik_transform_batch_submit_device(ptrs, lens, n, ws, hs, fs, qs, filt, threads, outs, olens, status,
                                                  ctypes.byref(ticket))
    else:
        ra = _request_opts(n, fits, orient, backgrounds, blurs, sharpens, overlays, adjusts=adjusts, pads=pads)
        st = lib.ik_transform_batch_submit_device_opts(ptrs, lens, n, ws, hs, ra, ctypes.sizeof(ra._type_), fs,
                                                       qs, filt, threads, outs, olens, status, ctypes.byref(ticket))
    if st:
        raise TransformError(_lib.last_error())
    return PendingBatch((keep, ptrs, lens, ws, hs, fs, qs, ra, overlays), outs, olens, status, ticket.value, n)


def resize_image(img: DynamicImage, w: Optional[int], h: Optional[int],
                 filter: FilterType = FilterType.Lanczos3, fit: FitMode = FitMode.contain) -> DynamicImage:
    """src/transform.rs:62-90 (Lanczos3; `filter` and `fit` are extensions: FitMode)."""
    if w is None and h is None:
        return img
    for v in (w, h):
        if v is not None and not 0 <= v <= 0xFFFFFFFF:
            raise InvalidArgument("dimension must be a u32")
    out = ctypes.c_void_p()
    st = _lib.load().ik_resize_fit(img._h, -1 if w is None else int(w), -1 if h is None else int(h),
                                   int(FitMode(fit)), int(filter), ctypes.byref(out))
    if st:
        _raise(st, "resize_image")
    return DynamicImage(out.value)


def encode_image(img: DynamicImage, fmt: ImageFormat, quality: int) -> bytes:
    """src/transform.rs:113-150.  quality is a u8, clamped to [1, 100]."""
    if not 0 <= int(quality) <= 255:
        raise InvalidArgument("quality must be a u8")
    lib = _lib.load()
    buf = _lib.u8p()
    n = ctypes.c_size_t()
    st = lib.ik_encode(img._h, ImageFormat(fmt).value, int(quality), ctypes.byref(buf), ctypes.byref(n))
    if st:
        raise TransformError(_lib.last_error())
    try:
        return ctypes.string_at(buf, n.value)
    finally:
        lib.ik_buf_free(buf)


def transform(data: bytes, w: Optional[int], h: Optional[int], fmt: ImageFormat, quality: int,
              filter: FilterType = FilterType.Lanczos3, fit: FitMode = FitMode.contain,
              orient=Orientation.stored, background=None, blur=None, sharpen=None, overlay=None, adjust=None,
              pad=None) -> bytes:
    """decode -> resize_image -> encode_image in one device-resident call; with orient
    (Orientation) the decoded image is turned first, and w, h and fit refer to the turned
    image; with background (0xRRGGBB, (r, g, b), "rrggbb" or "#rrggbb") an image that
    carries alpha is then composited onto that colour, before the resize; with blur (a
    sigma) or sharpen (a sigma, or (sigma, threshold)) the resized image is blurred or
    sharpened by the unsharp mask before it is encoded; with overlay (an Overlay, or a
    DynamicImage for an opaque centred mark) that watermark is composited last, on the
    pixels the encoder codes; with adjust (an Adjust) the resized image's colours are
    adjusted before the blur or sharpen and the watermark; with pad (a Pad) the result is
    placed on a canvas before the watermark, a Pad size of 0 being the side of the box (w,
    h): fit contain with Pad() returns exactly w x h (ik_transform_opts)."""
    bg = _background(background)
    fa = _filter_args(blur, sharpen)
    mark = _overlay(overlay)
    adj = _adjust(adjust)
    pd = _pad(pad)
    lib = _lib.load()
    b = bytes(data)
    buf = _lib.u8p()
    n = ctypes.c_size_t()
    o = _orient(orient)
    if pd is not None or adj is not None or mark is not None or fa[0] or fa[1] or bg != BG_NONE:
        # the smallest declared layout that holds what is set
        if pd is not None or adj is not None:
            ro = (_lib.RequestOpts5 if pd is not None else _lib.RequestOpts4)(int(FitMode(fit)), o, bg, *fa)
            if mark is not None:
                mark._fill(ro)
            if adj is not None:
                ro.adjust = adj._struct()
            if pd is not None:
                ro.pad = pd._struct()
        elif mark is not None:
            ro = _lib.RequestOpts3(int(FitMode(fit)), o, bg, *fa)
            mark._fill(ro)
        elif fa[0] or fa[1]:
            ro = _lib.RequestOpts2(int(FitMode(fit)), o, bg, *fa)
        else:
            ro = _lib.RequestOpts(int(FitMode(fit)), o, bg)
        st = lib.ik_transform_opts(b, len(b), -1 if w is None else int(w), -1 if h is None else int(h),
                                   ImageFormat(fmt).value, int(quality), int(filter), ctypes.byref(ro),
                                   ctypes.sizeof(ro), ctypes.byref(buf), ctypes.byref(n))
    elif o == Orientation.stored:
        st = lib.ik_transform_fit(b, len(b), -1 if w is None else int(w), -1 if h is None else int(h),
                                  int(FitMode(fit)), ImageFormat(fmt).value, int(quality), int(filter),
                                  ctypes.byref(buf), ctypes.byref(n))
    else:
        st = lib.ik_transform_oriented(b, len(b), -1 if w is None else int(w), -1 if h is None else int(h),
                                       int(FitMode(fit)), o, ImageFormat(fmt).value, int(quality), int(filter),
                                       ctypes.byref(buf), ctypes.byref(n))
    if st:
        raise TransformError(_lib.last_error())
    try:
        return ctypes.string_at(buf, n.value)
    finally:
        lib.ik_buf_free(buf)
