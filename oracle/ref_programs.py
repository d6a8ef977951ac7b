"""ORACLE (test infrastructure only, CPU only): execute the reference's own model programs without its dependencies.

The reference's model files (sde/integrators.py, sde/transforms.py, sde/example_models/fhn.py, sir.py) and the model cells
of its notebook (FitzHugh-Nagumo_example.ipynb) need a handful of functions of `symnum`, `jax.numpy` and `jax.lax`, none of
which is installed where this repository is tested.  This module provides stand-ins for exactly those functions, written
here on top of sympy, mpmath and NumPy, registers them in `sys.modules` for the duration of one call of `load()`, and loads
the reference's files by path from the reference directory -- unchanged, and without running `sde/__init__.py` (which
imports the Mici extensions).  What comes back are the reference's own functions.

Two number modes for every executed program (`with number_mode("mp")` / `"f64"`):
  mp    mpmath at DPS = 50 digits: the value of the recursion, for all purposes of a double-precision comparison;
  f64   Python / NumPy doubles: what the reference itself delivers in double precision.

Nothing derived from the reference is written anywhere by this module: no printed expression, no generated source, no
pickle.  The symbolic step functions are rebuilt in memory in every process (about two seconds).  The reference
directory is `$CHMC_REFERENCE_DIR`, by default DEFAULT_REFERENCE_DIR; `available()` says whether it can be used."""
import contextlib
import importlib.util
import json
import os
import sys
import types
import numpy as np

DEFAULT_REFERENCE_DIR = "/root/reference"
DPS = 50
MODEL_FILES = ("sde/integrators.py", "sde/transforms.py", "sde/example_models/fhn.py", "sde/example_models/sir.py")
NOTEBOOK = "FitzHugh-Nagumo_example.ipynb"
# names whose absence is the only accepted reason to skip a notebook cell: libraries that are not installed (the import
# cell, which fails at its first line) and the names that cell or a skipped cell would have bound
NOTEBOOK_ABSENT = ("mici", "mici_extensions", "plt", "arviz", "corner", "system", "integrator", "sampler", "states", "traces",
                   "final_states", "stats", "init_states", "rng_init", "generate_init_state", "trace_func", "summary",
                   "summary_vars", "x_seq_post", "x_seq_traces")
# what the model and data cells must have defined
NOTEBOOK_NAMES = ("drift_func", "diff_coeff", "strong_order_1p5_step", "forward_func", "obs_func", "generate_z", "generate_x_0",
                  "generate_from_model", "dim_x", "dim_z", "dim_v", "num_obs", "num_steps_per_obs", "obs_interval", "δ", "q_ref",
                  "x_seq_ref", "y_seq_ref", "z_ref", "x_0_ref")


def reference_dir():
    return os.environ.get("CHMC_REFERENCE_DIR", DEFAULT_REFERENCE_DIR)


def available():
    """(usable, reason): whether the reference's files and the two libraries the stand-ins are built on are present."""
    for name in ("sympy", "mpmath"):
        if importlib.util.find_spec(name) is None:
            return False, f"{name} is not installed"
    d = reference_dir()
    missing = [f for f in MODEL_FILES + (NOTEBOOK,) if not os.path.isfile(os.path.join(d, f))]
    if missing:
        return False, f"the reference directory {d} (CHMC_REFERENCE_DIR) lacks {missing[0]}"
    return True, ""


# ---------------------------------------------------------------------------------------------------------------------
# number modes

_MODE = ["f64"]


@contextlib.contextmanager
def number_mode(name):
    """Everything the loaded programs compute inside this block is computed in `name`: "mp" or "f64"."""
    import mpmath
    if name not in ("mp", "f64"):
        raise ValueError(name)
    saved = _MODE[0]
    _MODE[0] = name
    try:
        if name == "mp":
            with mpmath.workdps(DPS):
                yield
        else:
            with np.errstate(all="ignore"):
                yield
    finally:
        _MODE[0] = saved


def _mp():
    return _MODE[0] == "mp"


def _num(x):
    """One number of the current mode."""
    import mpmath
    if not _mp():
        return float(x)
    return x if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x)) if not isinstance(x, int) else mpmath.mpf(x)


class Arr(np.ndarray):
    """The array of both modes (float64, or objects holding mpf) with the one jax idiom the model files use: x.at[i].set(v)."""

    @property
    def at(self):
        return _At(self)


class _At:
    def __init__(self, a):
        self.a = a

    def __getitem__(self, idx):
        return _AtIndex(self.a, idx)


class _AtIndex:
    def __init__(self, a, idx):
        self.a, self.idx = a, idx

    def set(self, value):
        out = self.a.copy()
        out[self.idx] = value
        return out


def to_array(obj):
    """Numbers, nested sequences or arrays -> Arr of the current mode."""
    if _mp():
        a = np.array(obj.tolist() if isinstance(obj, np.ndarray) else obj, dtype=object)
        out = np.empty(a.shape, dtype=object)
        for i in np.ndindex(*a.shape):
            out[i] = _num(a[i])
        return out.view(Arr)
    return np.array(obj, dtype=np.float64).view(Arr)


def _elementwise(name):
    def f(x):
        import mpmath
        if not _mp():
            return getattr(np, name)(x)
        g = getattr(mpmath, name)
        if isinstance(x, np.ndarray):
            return to_array([g(_num(t)) for t in x.ravel()]).reshape(x.shape)
        return g(_num(x))
    f.__name__ = name
    return f


def _clip(x, a_min=None, a_max=None):
    x = to_array(x)
    out = x.copy()
    for i in np.ndindex(*x.shape):
        if a_min is not None and out[i] < a_min:
            out[i] = _num(a_min)
        if a_max is not None and out[i] > a_max:
            out[i] = _num(a_max)
    return out


def _select(pred, on_true, on_false):
    return on_true if pred else on_false


def _scan(f, init, xs):
    carry, ys = init, []
    for x in xs:
        carry, y = f(carry, x)
        ys.append(y)
    return carry, to_array(ys)


def _jax_modules():
    jax, jnp, lax = types.ModuleType("jax"), types.ModuleType("jax.numpy"), types.ModuleType("jax.lax")
    jnp.array = jnp.asarray = to_array
    jnp.exp, jnp.sqrt, jnp.log = _elementwise("exp"), _elementwise("sqrt"), _elementwise("log")
    jnp.clip = _clip
    jnp.concatenate = lambda arrays, axis=0: to_array(np.concatenate([to_array(a) for a in arrays], axis))
    jnp.split = lambda a, idx, axis=0: [to_array(p) for p in np.split(to_array(a), list(idx), axis)]
    jnp.reshape = lambda a, shape: to_array(a).reshape(shape)
    lax.select, lax.scan = _select, _scan
    jax.numpy, jax.lax = jnp, lax
    jax.config = types.SimpleNamespace(update=lambda *a, **k: None)
    return {"jax": jax, "jax.numpy": jnp, "jax.lax": lax}


# ---------------------------------------------------------------------------------------------------------------------
# symnum: arrays of sympy expressions, the three differential operators, numpify_func

class SymArray:
    """An array of sympy expressions with the methods the reference's files call."""
    __array_priority__ = 1000

    def __init__(self, a):
        self.a = np.array(a, dtype=object)

    shape = property(lambda s: s.a.shape)
    T = property(lambda s: SymArray(s.a.T))

    def __getitem__(self, i):
        r = self.a[i]
        return SymArray(r) if isinstance(r, np.ndarray) else r

    def __len__(self):
        return self.a.shape[0]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def flatten(self):
        return SymArray(self.a.flatten())

    def sum(self):
        import sympy
        return sympy.Add(*self.a.flatten())

    def _map(self, f):
        out = np.empty(self.a.shape, dtype=object)
        for i in np.ndindex(*self.a.shape):
            out[i] = f(self.a[i])
        return SymArray(out)

    def diff(self, *v):
        import sympy
        return self._map(lambda e: sympy.diff(e, *v))

    def subs(self, pairs):
        import sympy
        return self._map(lambda e: sympy.sympify(e).subs(pairs))

    def __neg__(self):
        return SymArray(-self.a)


def _raw(x):
    return x.a if isinstance(x, SymArray) else x


def _wrap(r):
    return SymArray(r) if isinstance(r, np.ndarray) else r


def _binary(name, op):
    setattr(SymArray, f"__{name}__", lambda s, o: _wrap(op(_raw(s), _raw(o))))
    setattr(SymArray, f"__r{name}__", lambda s, o: _wrap(op(_raw(o), _raw(s))))


_binary("add", lambda a, b: a + b)
_binary("sub", lambda a, b: a - b)
_binary("mul", lambda a, b: a * b)
_binary("truediv", lambda a, b: a / b)
_binary("pow", lambda a, b: a ** b)
_binary("matmul", lambda a, b: a @ b)


def sym_array(obj):
    import sympy

    def conv(o):
        if isinstance(o, SymArray):
            return conv(o.a.tolist())
        if isinstance(o, (list, tuple)):
            return [conv(e) for e in o]
        return sympy.sympify(o)
    return SymArray(conv(obj))


def _sym_elementwise(name):
    def f(x):
        import sympy
        g = getattr(sympy, name)
        return x._map(g) if isinstance(x, SymArray) else g(sympy.sympify(x))
    return f


def named_array(name, shape):
    import sympy
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    a = np.empty(shape, dtype=object)
    for i in np.ndindex(*shape):
        a[i] = sympy.Symbol(f"{name}[{','.join(map(str, i))}]", real=True)
    return SymArray(a)


def jacobian(func):
    """d func / d (first argument), [outputs, inputs]."""
    import sympy

    def at(*args):
        out, x = sym_array(func(*args)).a.flatten(), args[0].a.flatten()
        return SymArray([[sympy.diff(o, xi) for xi in x] for o in out])
    return at


def jacobian_vector_product(func):
    return lambda *args: lambda v: jacobian(func)(*args) @ sym_array(v)


def matrix_hessian_product(func):
    """m -> sum_ij d^2 func / dx_i dx_j m_ij, per output."""
    import sympy

    def at(*args):
        out, x = sym_array(func(*args)).a.flatten(), args[0].a.flatten()

        def mhp(m):
            m = sym_array(m).a
            return SymArray([sympy.Add(*[sympy.diff(o, xi, xj) * m[i, j] for i, xi in enumerate(x) for j, xj in enumerate(x)])
                             for o in out])
        return mhp
    return at


class Numpified:
    """numpify_func's result: the symbolic function of array and scalar arguments, evaluated in the current number mode."""

    def __init__(self, func, shapes):
        import sympy
        self.args = [sympy.Symbol(f"s{k}", positive=True) if s is None else named_array(f"a{k}", s)
                     for k, s in enumerate(shapes)]
        self.expr = sym_array(func(*self.args))
        self.symbols = [s for a in self.args for s in (a.a.flatten() if isinstance(a, SymArray) else [a])]
        self.compiled = {}

    def __call__(self, *values):
        import sympy
        mode = _MODE[0]
        if mode not in self.compiled:
            self.compiled[mode] = sympy.lambdify(self.symbols, list(self.expr.a.flatten()),
                                                 modules="mpmath" if mode == "mp" else "numpy")
        flat = []
        for a, v in zip(self.args, values):
            flat += [_num(t) for t in np.ravel(v)] if isinstance(a, SymArray) else [_num(v)]
        return to_array(self.compiled[mode](*flat)).reshape(self.expr.shape)


def _symnum_modules():
    symnum, snp = types.ModuleType("symnum"), types.ModuleType("symnum.numpy")
    diffops, symbolic = types.ModuleType("symnum.diffops"), types.ModuleType("symnum.diffops.symbolic")
    snp.array = sym_array
    snp.exp, snp.sqrt, snp.log = _sym_elementwise("exp"), _sym_elementwise("sqrt"), _sym_elementwise("log")
    symbolic.jacobian, symbolic.jacobian_vector_product = jacobian, jacobian_vector_product
    symbolic.matrix_hessian_product = matrix_hessian_product
    symnum.numpy, symnum.diffops, diffops.symbolic = snp, diffops, symbolic
    symnum.named_array = named_array
    symnum.numpify_func = lambda func, *shapes, numpy_module=None: Numpified(func, shapes)
    return {"symnum": symnum, "symnum.numpy": snp, "symnum.diffops": diffops, "symnum.diffops.symbolic": symbolic}


# ---------------------------------------------------------------------------------------------------------------------
# loading

@contextlib.contextmanager
def _stand_ins(extra):
    mods = {**_symnum_modules(), **_jax_modules(), **extra}
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        yield mods
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _load_file(name, path, registry):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    registry.append(name)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _run_notebook_cells(path, mods):
    """The notebook's code cells in order in one namespace.  The names its import cell would bind are bound to the
    stand-ins beforehand; IPython shell lines are dropped; a cell that raises ImportError or NameError (it needs mici, the
    Mici extensions or a plotting library) is skipped.  Returns (namespace, indices of the cells that ran)."""
    with open(path, encoding="utf-8") as f:
        cells = json.load(f)["cells"]
    ns = dict(symnum=mods["symnum"], diffops=mods["symnum.diffops.symbolic"], snp=mods["symnum.numpy"], onp=np,
              jax=mods["jax"], lax=mods["jax.lax"], jnp=mods["jax.numpy"], config=mods["jax"].config,
              __name__="reference_notebook")
    ran, skipped = [], {}
    for k, cell in enumerate(cells):
        if cell["cell_type"] != "code":
            continue
        lines = "".join(cell["source"]).split("\n")
        src = "\n".join((ln[:len(ln) - len(ln.lstrip())] + "pass") if ln.lstrip()[:1] in ("!", "%") else ln for ln in lines)
        try:
            exec(compile(src, f"<notebook cell {k}>", "exec"), ns)
            ran.append(k)
        except (ImportError, NameError) as e:
            skipped[k] = f"{type(e).__name__}: {e}"
    # A skipped cell must be one that needs what is not here -- never a model cell dropped by a gap in the stand-ins: every
    # skip names one of the absent libraries, and every name the model and data cells define is there
    for k, why in skipped.items():
        if not any(f"'{name}'" in why for name in NOTEBOOK_ABSENT):
            raise RuntimeError(f"notebook cell {k} was skipped for a reason other than an absent library: {why}")
    missing = [n for n in NOTEBOOK_NAMES if n not in ns]
    if missing:
        raise RuntimeError(f"the notebook's cells did not define {missing}; skipped cells: {skipped}")
    return ns, ran, skipped


_LOADED = {}


def load():
    """The reference's programs: a namespace with `fhn`, `sir` (the loaded modules), `nb` (the notebook's namespace, its data
    cells run in f64 mode) and `models`: name -> dict(forward_func, generate_z, generate_x_0, obs_func, generate_sigma_y or
    None, dim_z, dim_x, dim_v, dim_v_0).  Loaded once per process and reference directory."""
    d = reference_dir()
    if d in _LOADED:
        return _LOADED[d]
    ok, why = available()
    if not ok:
        raise RuntimeError(why)
    sde, models_pkg = types.ModuleType("sde"), types.ModuleType("sde.example_models")
    sde.__path__, models_pkg.__path__ = [], []  # bare packages: sde/__init__.py is not executed
    registry, write_bytecode = [], sys.dont_write_bytecode
    sys.dont_write_bytecode = True  # nothing compiled from the reference is left behind, wherever it lies
    try:
        with _stand_ins({"sde": sde, "sde.example_models": models_pkg}) as mods, number_mode("f64"):
            try:
                sde.integrators = _load_file("sde.integrators", os.path.join(d, MODEL_FILES[0]), registry)
                sde.transforms = _load_file("sde.transforms", os.path.join(d, MODEL_FILES[1]), registry)
                sde.example_models = models_pkg
                fhn = models_pkg.fhn = _load_file("sde.example_models.fhn", os.path.join(d, MODEL_FILES[2]), registry)
                sir = models_pkg.sir = _load_file("sde.example_models.sir", os.path.join(d, MODEL_FILES[3]), registry)
                nb, ran, skipped = _run_notebook_cells(os.path.join(d, NOTEBOOK), mods)
            finally:
                for name in registry:
                    sys.modules.pop(name, None)
    finally:
        sys.dont_write_bytecode = write_bytecode

    def entry(ns, sigma_y=True):
        g = (lambda k: ns[k]) if isinstance(ns, dict) else (lambda k: getattr(ns, k))
        dim_x, dim_z = g("dim_x"), g("dim_z")
        return dict(forward_func=g("forward_func"), generate_z=g("generate_z"), generate_x_0=g("generate_x_0"),
                    obs_func=g("obs_func"), generate_sigma_y=g("generate_σ_y") if sigma_y else None, dim_x=dim_x, dim_z=dim_z,
                    dim_v=g("dim_v"), dim_v_0=dim_x if isinstance(ns, dict) else g("dim_v_0"))

    out = types.SimpleNamespace(fhn=fhn, sir=sir, nb=nb, nb_cells_run=ran, nb_cells_skipped=skipped,
                                models={"fhn": entry(fhn), "sir": entry(sir), "fhn_nb": entry(nb, sigma_y=False)})
    _LOADED[d] = out
    return out
