"""
The cases that hold the element-wise device operators (``hdem_elementwise_dev`` behind
``backend.elementwise_dev`` and the ``apply_device`` of the six filters of
``filters/simple_filters.py``) to NumPy's own results, and a check that these cases can
tell NumPy from the arithmetic the device path used to do.  No GPU is needed here;
tests/test_gpu_elementwise.py imports the generator and the comparison and runs the cases
on the device.

The reference is ``filter.apply`` on host arrays: one NumPy ufunc each.  A uint8 raster is
the device form of NumPy's bool / int64 masks, so a uint8 image or operand reaches the
reference as int64.

The module docstring of ``simple_filters`` promises "the same operator" on the device.
Where the device path could break that promise (read from the code, and modelled below as
``model_in_double``):

* a float32 raster with a Python float that float32 cannot hold: NumPy rounds the scalar
  to float32 and works in float32, the kernel took the double;
* a float32 raster with an int64 raster or an ``np.float64`` scalar: NumPy gives float64,
  the type rule gave float32;
* a host array as operand: an int64 array above 2^24 was cast to float32 on the way up;
* two uint8 rasters multiplied: the value to hold is up to 255 * 255, the output was uint8;
* special values: NaN, +-inf, +-0.0, the smallest float32 denormal, FLT_MAX, and for every
  scalar ``s`` the cell ``np.float32(s)`` with its two float32 neighbours (``a > 0.1`` is
  False in NumPy for the cell equal to ``np.float32(0.1)``).
"""
import numpy as np

import hydrodem_amd as hd

DEVICE_TYPES = (np.float32, np.float64, np.uint8, np.int64)
SHAPES = [(1, n) for n in range(1, 10)] + [(1, 1023), (1, 1024), (1, 1025), (37, 53)]
PY_SCALARS = (1, 4, 2.5, 0.1, 1.1, 1 / 3)
INT_LIMIT = 2 ** 53                 # the kernel's documented contract for integers
INT_SPAN = 2 ** 26                  # |integer cell| <= 2^26: a product stays within 2^52

FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.float32(1e-45)      # the smallest float32 denormal, 2^-149


def _specials():
    values = [np.nan, np.inf, -np.inf, 0.0, -0.0, float(DENORM_MIN), float(FLT_MAX)]
    for s in PY_SCALARS:
        at = np.float32(s)
        values += [float(np.nextafter(at, np.float32(-np.inf))), float(at),
                   float(np.nextafter(at, np.float32(np.inf)))]
    return values


SPECIALS = _specials()              # every one is a float32 value, so exact in float64 too
INT_SPECIALS = [0, 1, -1, 255, 256, 2 ** 24 + 1, -(2 ** 24 + 1), INT_SPAN, -INT_SPAN]


class OnDevice:  # pylint: disable=too-few-public-methods
    """An operand that the device side uploads as a ``DeviceRaster`` (the host side reads
    ``.array``); a bare ndarray operand stays a host array on both sides."""

    def __init__(self, array):
        self.array = array


FILTERS = {
    "LowerThan": lambda v: hd.LowerThan(value=v),
    "GreaterThan": lambda v: hd.GreaterThan(value=v),
    "ProductFilter": lambda v: hd.ProductFilter(factor=v),
    "AdditionFilter": lambda v: hd.AdditionFilter(addend=v),
    "SubtractionFilter": lambda v: hd.SubtractionFilter(minuend=v),
}
for _name, _factory in FILTERS.items():
    _factory.__name__ = _name


def boolean_to_integer(_operand=None):
    return hd.BooleanToInteger()


boolean_to_integer.__name__ = "BooleanToInteger"


def _plant(a, values, rng, turn):
    """Write ``values`` into ``a``: all of them at seeded places (the last cell among them)
    where they fit, else the next ``a.size`` of them in turn, so that the small shapes
    together carry every one."""
    flat = a.reshape(-1)
    if flat.size > len(values):
        where = rng.choice(flat.size - 1, len(values) - 1, replace=False)
        flat[where] = values[:-1]
        flat[-1] = values[-1]
    else:
        for k in range(flat.size):
            flat[k] = values[(turn + k) % len(values)]


def image_of(dtype, shape, seed):
    """A raster of ``dtype``: seeded random cells plus the planted ones."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([seed, shape[0], shape[1], dtype.num])
    size = shape[0] * shape[1]
    turn = 7 * (size + seed)
    if dtype.kind == "f":
        a = (rng.random(shape) * 9).astype(dtype)
        _plant(a, SPECIALS, rng, turn)
    elif dtype == np.uint8:
        a = rng.permutation(np.arange(max(size, 256)) % 256)[:size].astype(np.uint8)
        a = a.reshape(shape)
        if size >= 2:
            a.reshape(-1)[[0, -1]] = 255, 0
    else:
        a = rng.integers(-INT_SPAN, INT_SPAN + 1, shape, dtype=np.int64)
        _plant(a, INT_SPECIALS, rng, turn)
    return a


def planted(image):
    """Where ``image`` holds one of the special float values."""
    if image.dtype.kind != "f":
        return np.zeros(image.shape, bool)
    finite = np.array([v for v in SPECIALS if v == v], dtype=image.dtype)
    return np.isnan(image) | np.isin(image, finite)


def _operands():
    """name -> operand(shape): the operand axis of the cases."""
    ops = {}
    for s in PY_SCALARS:
        ops[f"py {type(s).__name__} {s:.3g}"] = lambda shape, s=s: s
    ops["np.float32(0.1)"] = lambda shape: np.float32(0.1)
    ops["np.float64(0.1)"] = lambda shape: np.float64(0.1)
    for t in DEVICE_TYPES:
        name = np.dtype(t).name
        ops[f"device {name}"] = lambda shape, t=t: OnDevice(image_of(t, shape, 11))
        ops[f"host {name}"] = lambda shape, t=t: image_of(t, shape, 12)
    ops["host bool"] = lambda shape: image_of(np.uint8, shape, 13) % 2 == 1
    ops["host int64 above 255"] = lambda shape: 256 + image_of(np.uint8, shape, 14).astype(np.int64) * 3
    ops["host int64 above 2^24"] = lambda shape: (2 ** 24 + 1 + 2 * image_of(np.uint8, shape, 15).astype(np.int64))
    return ops


OPERANDS = _operands()


def cases(dtype=None, operand=None):
    """(filter_factory, image, operand) triples: every shape, image type, operand and
    filter, or those of one image ``dtype`` / one name of ``OPERANDS``.  The factory makes
    the filter from the operand in the form a side needs it (an uploaded raster on the
    device, host arrays for the reference).  ``BooleanToInteger`` has no operand and comes
    once per image, with the operand ``None``, under the Python int 1."""
    for t in DEVICE_TYPES if dtype is None else (dtype,):
        for name, make in OPERANDS.items():
            if operand is not None and name != operand:
                continue
            for shape in SHAPES:
                image = image_of(t, shape, 1)
                other = make(shape)
                for factory in FILTERS.values():
                    yield factory, image, other
                if name == "py int 1":
                    yield boolean_to_integer, image, None


def host_form(x):
    """What the reference takes for ``x``: the array of a device operand, int64 for uint8."""
    if isinstance(x, OnDevice):
        x = x.array
    if isinstance(x, np.ndarray) and x.dtype == np.uint8:
        return x.astype(np.int64)
    return x


def expected(factory, image, operand):
    """The host ``apply`` (one NumPy ufunc) of the filter on the host arrays."""
    with np.errstate(all="ignore"):
        return factory(host_form(operand)).apply(host_form(image))


def differing(got, want):
    """Cells of ``got`` that are not ``want``'s after the cast to ``want``'s type: by bytes
    (the sign of zero counts), NaN equal to NaN, and for an integer ``want`` a value that
    the cast changed differs."""
    with np.errstate(all="ignore"):
        cast = got.astype(want.dtype)
        if want.dtype.kind == "f":
            bits = np.dtype(f"u{want.dtype.itemsize}")
            return (cast.view(bits) != want.view(bits)) & ~(np.isnan(cast) & np.isnan(want))
        return (cast != want) | (cast.astype(got.dtype) != got)


def same(got, want):
    """``got`` (from the device) is ``want`` (from NumPy): equal shapes, no differing cell,
    and the type NumPy's stands for -- the same float type, uint8 for bool, and for an
    integer type any device type that holds every value."""
    if got.shape != want.shape:
        return False
    if want.dtype.kind == "f":
        if got.dtype != want.dtype:
            return False
    elif want.dtype == bool:
        if got.dtype != np.uint8:
            return False
    elif want.dtype.kind not in "iu" or got.dtype not in DEVICE_TYPES:
        return False
    return not differing(got, want).any()


def model_in_double(factory, image, operand):
    """What the device path computed before it was held to NumPy, as plain NumPy: the
    operand cast as ``apply_device`` cast it, the arithmetic in float64 with the scalar
    as passed (``float(operand)``), one cast to the type ``elementwise_dev`` picked."""
    op = factory(0).device_op
    if factory is boolean_to_integer:
        operand = 1
    raster = None
    if isinstance(operand, OnDevice):
        raster = operand.array
    elif isinstance(operand, np.ndarray):
        raster = operand
        if raster.dtype == bool or (raster.dtype.kind in "iu" and raster.min() >= 0 and
                                    raster.max() <= 255):
            raster = raster.astype(np.uint8)
        elif raster.dtype != np.float64:
            raster = raster.astype(np.float32)
    kinds = [image.dtype] + ([raster.dtype] if raster is not None else [])
    if op in (hd.backend.EW_GT, hd.backend.EW_LT):
        out = np.uint8
    elif any(k == np.float64 for k in kinds):
        out = np.float64
    elif op == hd.backend.EW_MUL and all(k == np.uint8 for k in kinds) and \
            (raster is not None or float(operand) in (0.0, 1.0)):
        out = np.uint8
    else:
        out = np.float32
    with np.errstate(all="ignore"):
        x = image.astype(np.float64)
        y = raster.astype(np.float64) if raster is not None else np.float64(float(operand))
        r = {hd.backend.EW_MUL: lambda: y * x, hd.backend.EW_ADD: lambda: y + x,
             hd.backend.EW_RSUB: lambda: y - x,
             hd.backend.EW_GT: lambda: (x > y).astype(np.float64),
             hd.backend.EW_LT: lambda: (x < y).astype(np.float64)}[op]()
        if out == np.uint8:                     # (an out-of-range byte: taken as wrapped)
            return r.astype(np.int64).astype(np.uint8)
        return r.astype(out)


def _inexact(s):
    return isinstance(s, float) and float(np.float32(s)) != s


# the groups of divergences that pass through hdem_elementwise_dev: which cases belong
GROUPS = {
    "float32 raster, Python float that float32 cannot hold":
        lambda f, image, operand: image.dtype == np.float32 and type(operand) is float
        and _inexact(operand),
    "float32 raster with an int64 raster or an np.float64 scalar":
        lambda f, image, operand: image.dtype == np.float32 and (
            isinstance(operand, np.float64) or
            (isinstance(operand, OnDevice) and operand.array.dtype == np.int64)),
    "host array as operand, int64 above 2^24":
        lambda f, image, operand: isinstance(operand, np.ndarray) and
        operand.dtype == np.int64 and operand.min() > 2 ** 24,
    "two uint8 rasters multiplied":
        lambda f, image, operand: image.dtype == np.uint8 and f.__name__ == "ProductFilter"
        and isinstance(operand, OnDevice) and operand.array.dtype == np.uint8,
    "special values":
        lambda f, image, operand: image.dtype.kind == "f",
}


def test_the_cases_tell_the_old_double_arithmetic_from_numpy():
    """In every group at least one case separates the model of the old device path from
    NumPy -- and in the group of the special values it does so at a planted cell."""
    caught = dict.fromkeys(GROUPS, 0)
    for factory, image, operand in cases():
        groups = [g for g, member in GROUPS.items() if member(factory, image, operand)]
        if not groups:
            continue
        want = expected(factory, image, operand)
        model = model_in_double(factory, image, operand)
        if same(model, want):
            continue
        at_planted = model.shape == want.shape and (differing(model, want) & planted(image)).any()
        for g in groups:
            if g != "special values" or at_planted:
                caught[g] += 1
    assert all(caught.values()), caught


def test_the_model_is_numpy_where_the_old_path_was_right():
    """The model is not merely different everywhere: float64 rasters with Python scalars
    and float32 rasters with scalars that float32 holds were NumPy's already."""
    for factory, image, operand in cases(dtype=np.float64):
        if type(operand) in (int, float) and factory is not boolean_to_integer:
            assert same(model_in_double(factory, image, operand),
                        expected(factory, image, operand)), (factory.__name__, operand)
    for factory, image, operand in cases(dtype=np.float32, operand="py float 2.5"):
        assert same(model_in_double(factory, image, operand),
                    expected(factory, image, operand)), factory.__name__


def test_integers_stay_within_the_documented_2_to_the_53():
    for factory, image, operand in cases():
        arrays = [image, host_form(operand), expected(factory, image, operand)]
        for a in arrays:
            a = np.asarray(a)
            if a.dtype.kind in "iu":
                assert np.abs(a.astype(np.int64)).max() <= INT_LIMIT, (factory.__name__, a.dtype)


def test_expected_raises_for_no_case_and_every_axis_is_there():
    seen = set()
    for factory, image, operand in cases():
        want = expected(factory, image, operand)
        assert want.shape == image.shape
        seen.add((factory.__name__, image.dtype.name, image.shape))
    assert len(seen) == 6 * len(DEVICE_TYPES) * len(SHAPES)
    for t in (np.float32, np.float64):            # every special is planted somewhere
        bits = np.dtype(f"u{np.dtype(t).itemsize}")
        have = set()
        for shape in SHAPES:
            have |= set(image_of(t, shape, 1).view(bits).reshape(-1).tolist())
        assert {int(np.array(v, t).view(bits)) for v in SPECIALS} <= have
    assert set(np.concatenate([image_of(np.uint8, s, 1).reshape(-1) for s in SHAPES])) == \
        set(range(256))


def test_same_counts_type_sign_of_zero_and_nan():
    z = np.array([[0.0, np.nan, 1.5]], np.float32)
    assert same(z.copy(), z)
    assert not same(np.array([[-0.0, np.nan, 1.5]], np.float32), z)
    assert not same(z.astype(np.float64), z) and not same(z[:, :2], z)
    m = np.array([[True, False]])
    assert same(m.astype(np.uint8), m) and not same(m.astype(np.int64), m)
    i = np.array([[400, -1]], np.int64)
    assert same(i.astype(np.float64), i) and same(i.copy(), i)
    assert not same(i.astype(np.uint8), i) and not same(np.array([[400.5, -1]]), i)
