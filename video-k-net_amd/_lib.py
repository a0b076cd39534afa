"""ctypes binding of libvkn.so, computed from its C ABI in include/vkn.h, + the hipcc build recipe.

The library is built IN-TREE (`video-k-net_amd/lib/libvkn.so`) so that it travels with the repo snapshot to the GPU
box; there is no CPU fallback: if the library is missing every op raises `VknLibraryError`.
"""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIBDIR = os.path.join(HERE, 'lib')
LIBPATH = os.path.join(LIBDIR, 'libvkn.so')
SOURCES = ('vkn_gather.hip', 'vkn_update.hip', 'vkn_decode.hip', 'vkn_fused.hip', 'vkn_init.hip', 'vkn_panoptic.hip', 'vkn_merge.hip', 'vkn_assign.hip', 'vkn_assign_lr.hip', 'vkn_tracker.hip', 'vkn_loss.hip', 'vkn_chain.hip', 'vkn_chain_h2.hip', 'vkn_ksplit.hip', 'vkn_train.hip', 'vkn_fpn.hip', 'vkn_optim.hip', 'vkn_tracktail.hip', 'vkn_trackloss.hip', 'vkn_gtprep.hip', 'vkn_api.hip')
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'vkn.h')
TRACK_HEADER = os.path.join(os.path.dirname(HERE), 'include', 'vkn_track.h')     # second part of the ABI: the tracking tail
TRACK_TRAIN_HEADER = os.path.join(os.path.dirname(HERE), 'include', 'vkn_track_train.h')     # third part: the tracking loss
GT_HEADER = os.path.join(os.path.dirname(HERE), 'include', 'vkn_gt.h')     # fourth part: the ground truth of a training step
DECODE_HEADER = os.path.join(os.path.dirname(HERE), 'include', 'vkn_decode.h')     # fifth part: the decode on a workgroup budget


class VknLibraryError(RuntimeError):
    pass


class VknError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'libvkn error {code}: {msg}')
        self.code = code


# ---- the reader of include/vkn.h.  Everything here that restates the C ABI (prototypes, struct mirrors, constants) is computed from
#      the header by it, once per process.  It knows exactly the C subset the header is written in and refuses the rest.
_SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'unsigned int': ctypes.c_uint, 'size_t': ctypes.c_size_t,
            'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong}
_POINTEES = {'void', 'char', 'unsigned char', 'int64_t'}     # types the header only ever points at
_DECLARATOR = re.compile(r'([\w\s]*?)\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[(\w+)\])?')


def _int(text, consts, where):
    """`64`, `1u`, `0x000600`, `(-3)`, `(VKN_A | VKN_B)` -> int"""
    total = 0
    for term in text.strip('() \t').split('|'):
        term = term.strip()
        if not (term in consts or re.fullmatch(r'-?\d+|\d+u|0x[0-9a-fA-F]+', term)):
            raise VknLibraryError(f'include/vkn.h: {where}: {text.strip()!r} is not an integer this binding can read')
        total |= consts[term] if term in consts else int(term.rstrip('u'), 0)
    return total


def _declaration(decl, known, consts, where):
    """One declaration, `const float *a, *b[VKN_N]` -> [(name, base type, pointer depth, array length or None)]"""
    out, base = [], None
    for part in decl.split(','):
        m = _DECLARATOR.fullmatch(part.strip())
        words = [w for w in m.group(1).split() if w != 'const'] if m else []
        base = ' '.join(words) or base
        if not m or bool(words) == bool(out) or base not in known:      # the type comes first, and only first
            raise VknLibraryError(f'include/vkn.h: {where}: cannot read the declaration {" ".join(decl.split())!r}')
        out.append((m.group(3), base, m.group(2).count('*'), m.group(4) and _int(m.group(4), consts, where)))
    return out


def read_header(text):
    """(prototypes, structs, constants) of a header written in vkn.h's C subset:
    prototypes {function: ((base type, pointer depth) of the result, [(parameter, base type, pointer depth)])},
    structs {name: [(field, base type, pointer depth, array length or None)]}, constants {VKN_*: int}; all in the header's order.
    Raises VknLibraryError naming the declaration it cannot read."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    consts, structs, protos, known = {}, {}, {}, set(_SCALARS) | _POINTEES
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(VKN_\w+)(.*)$', text, flags=re.M):
        if value.strip():                                               # (the include guard has no value)
            consts[name] = _int(value, consts, name)
    text = re.sub(r'#ifdef __cplusplus.*?#endif', '', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)

    def struct(m):
        structs[m.group(2)] = [f for d in m.group(1).split(';') if d.strip() for f in _declaration(d, known, consts, m.group(2))]
        known.add(m.group(2))
        return ''
    text = re.sub(r'typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;', struct, text)
    for decl in filter(None, (' '.join(d.split()) for d in text.split(';'))):
        m = re.fullmatch(r'([\w\s\*]+?)\b(vkn_\w+)\s*\(([^()]*)\)', decl)
        if not m:
            raise VknLibraryError(f'include/vkn.h: cannot read the declaration {decl[:120]!r}')
        (_, rbase, rdepth, _), = _declaration(m.group(1) + ' result', known, consts, m.group(2))
        params = [] if m.group(3).strip() == 'void' else [q for p in m.group(3).split(',') for q in _declaration(p, known, consts, m.group(2))]
        if any(length is not None for *_, length in params):
            raise VknLibraryError(f'include/vkn.h: {m.group(2)}: array parameters are not supported')
        protos[m.group(2)] = ((rbase, rdepth), [q[:3] for q in params])
    return protos, structs, consts


with open(HEADER) as _f:
    PROTOS, STRUCTS, CONSTS = read_header(_f.read())
SYMBOLS = tuple(PROTOS)                     # every symbol include/vkn.h declares
with open(HEADER) as _f, open(TRACK_HEADER) as _g:          # vkn_track.h builds on vkn.h's structs: read behind it, keep what it adds
    _protos, _, _consts = read_header(_f.read() + '\n' + _g.read())
TRACK_PROTOS = {k: v for k, v in _protos.items() if k not in PROTOS}
TRACK_SYMBOLS = tuple(TRACK_PROTOS)         # every symbol include/vkn_track.h declares
CONSTS.update({k: v for k, v in _consts.items() if k not in CONSTS})
with open(HEADER) as _f, open(TRACK_HEADER) as _g, open(TRACK_TRAIN_HEADER) as _h:      # vkn_track_train.h: read behind the other two
    _protos, _structs, _consts = read_header(_f.read() + '\n' + _g.read() + '\n' + _h.read())
TRACK_TRAIN_PROTOS = {k: v for k, v in _protos.items() if k not in PROTOS and k not in TRACK_PROTOS}
TRACK_TRAIN_SYMBOLS = tuple(TRACK_TRAIN_PROTOS)         # every symbol include/vkn_track_train.h declares
TRACK_TRAIN_STRUCTS = {k: v for k, v in _structs.items() if k not in STRUCTS}
CONSTS.update({k: v for k, v in _consts.items() if k not in CONSTS})
with open(HEADER) as _f, open(TRACK_HEADER) as _g, open(TRACK_TRAIN_HEADER) as _h, open(GT_HEADER) as _i:      # vkn_gt.h: behind the other three
    _protos, _structs, _consts = read_header(_f.read() + '\n' + _g.read() + '\n' + _h.read() + '\n' + _i.read())
GT_PROTOS = {k: v for k, v in _protos.items() if k not in PROTOS and k not in TRACK_PROTOS and k not in TRACK_TRAIN_PROTOS}
GT_SYMBOLS = tuple(GT_PROTOS)               # every symbol include/vkn_gt.h declares
GT_STRUCTS = {k: v for k, v in _structs.items() if k not in STRUCTS and k not in TRACK_TRAIN_STRUCTS}
CONSTS.update({k: v for k, v in _consts.items() if k not in CONSTS})
with open(DECODE_HEADER) as _f:            # vkn_decode.h: prototypes on plain types only, read on its own
    DECODE_PROTOS, _, _ = read_header(_f.read())
DECODE_SYMBOLS = tuple(DECODE_PROTOS)       # every symbol include/vkn_decode.h declares
GT_MAX_IMAGES = CONSTS['VKN_GT_MAX_IMAGES']
GT_MAX_CLASSES = CONSTS['VKN_GT_MAX_CLASSES']
GT_MAX_IDS = CONSTS['VKN_GT_MAX_IDS']
TRACK_LOSS_MAX_ROWS = CONSTS['VKN_TRACK_LOSS_MAX_ROWS']
TRACK_MAX_K = CONSTS['VKN_TRACK_MAX_K']
MAX_FCS = CONSTS['VKN_MAX_FCS']
SPLIT_MAX_ITEMS = CONSTS['VKN_SPLIT_MAX_ITEMS']
DW_MAX_ITEMS = CONSTS['VKN_DW_MAX_ITEMS']
ADAMW_GROUP_ROW = CONSTS['VKN_ADAMW_GROUP_ROW']     # lr, weight_decay, beta1, beta2, eps (fp64)
MIRRORS = {}                                # struct name -> ctypes.Structure, in the header's order
TRACK_TRAIN_MIRRORS = {}                    # the structs of include/vkn_track_train.h, kept apart: MIRRORS is what vkn.h declares
GT_MIRRORS = {}                             # the structs of include/vkn_gt.h, kept apart in the same way


def _ctype(base, depth, where, result=False):
    """Scalars by value; `const char*` results as bytes; a pointer to a mirrored struct typed; every other pointer (device memory, for the
    most part) travels as an integer."""
    if depth == 0 and base in _SCALARS:
        return _SCALARS[base]
    if depth == 1 and base == 'char' and result:
        return ctypes.c_char_p
    if depth == 1 and base in MIRRORS:
        return ctypes.POINTER(MIRRORS[base])
    if depth == 1 and base in TRACK_TRAIN_MIRRORS:
        return ctypes.POINTER(TRACK_TRAIN_MIRRORS[base])
    if depth == 1 and base in GT_MIRRORS:
        return ctypes.POINTER(GT_MIRRORS[base])
    if depth == 0:
        raise VknLibraryError(f'include/vkn.h: {where}: {base!r} by value has no ctypes counterpart here')
    return ctypes.c_void_p


for _name, _fields in STRUCTS.items():
    MIRRORS[_name] = type(_name, (ctypes.Structure,), {
        '__doc__': f'Mirror of include/vkn.h: {_name} (device pointers as integers).',
        '_fields_': [(f, _ctype(b, d, _name) * n if n else _ctype(b, d, _name)) for f, b, d, n in _fields]})
for _name, _fields in TRACK_TRAIN_STRUCTS.items():
    TRACK_TRAIN_MIRRORS[_name] = type(_name, (ctypes.Structure,), {
        '__doc__': f'Mirror of include/vkn_track_train.h: {_name}.',
        '_fields_': [(f, _ctype(b, d, _name) * n if n else _ctype(b, d, _name)) for f, b, d, n in _fields]})
globals().update(TRACK_TRAIN_MIRRORS)       # VknTrackLossCfg
for _name, _fields in GT_STRUCTS.items():
    GT_MIRRORS[_name] = type(_name, (ctypes.Structure,), {
        '__doc__': f'Mirror of include/vkn_gt.h: {_name} (device pointers as integers).',
        '_fields_': [(f, _ctype(b, d, _name) * n if n else _ctype(b, d, _name)) for f, b, d, n in _fields]})
globals().update(GT_MIRRORS)                # VknGtImage
# importable by name: VknDims, VknStageWeights, VknSplitItem, VknDwItem, VknUpdatorNorms, VknUpdatorNormGrads, VknPanopticCfg, VknAssignCfg,
# VknAssignProblem, VknLsapProblem, VknTailImage, VknTailCfg, VknAdamwItem, VknTrackerCfg
globals().update(MIRRORS)

# The pointer parameters that do NOT follow _ctype's rule: (function, parameter) -> ctypes type.
POINTER_EXCEPTIONS = {
    ('vkn_adamw_flat_f32', 'items'): ctypes.c_void_p,       # the VknAdamwItem array lives in DEVICE memory: callers pass tensor.data_ptr()
    ('vkn_sum_n_f32', 'srcs'): ctypes.POINTER(ctypes.c_void_p),                   # a HOST array of device pointers, (c_void_p * n)(...)
    ('vkn_qd_tracker_state_layout', 'offsets12'): ctypes.POINTER(ctypes.c_size_t),  # a HOST array the call fills, (c_size_t * 12)()
}
for _fn, _p in POINTER_EXCEPTIONS:
    if _p not in [q[0] for q in PROTOS.get(_fn, ((), ()))[1]]:
        raise VknLibraryError(f'POINTER_EXCEPTIONS names {_fn}({_p}), which include/vkn.h does not declare')

DEBUG_LIBPATH = os.path.join(LIBDIR, 'libvkn_debug.so')


def _hipcc(args, verbose=False, what='hipcc'):
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', *args]
    if verbose:
        print(' '.join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise VknLibraryError(f'{what} failed:\n' + r.stdout + r.stderr)


def _shared_deps(debug):
    """What every object depends on besides csrc/: the public header and, in the debug build, the kernel variants it #includes."""
    exp = os.path.join(os.path.dirname(HERE), 'tools', 'experiments')
    return [HEADER, TRACK_HEADER, TRACK_TRAIN_HEADER, GT_HEADER, DECODE_HEADER] + ([os.path.join(exp, f) for f in os.listdir(exp)] if debug and os.path.isdir(exp) else [])


def _stale(path=None):
    path = path or LIBPATH
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + _shared_deps(path == DEBUG_LIBPATH)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _compile_objects(objdir, extra=(), force=False, verbose=False):
    """One `hipcc -c` per source, in parallel, re-using objects newer than every header and their own source (no cross-file device
    symbols exist, so plain separate compilation links)."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')] + _shared_deps('-DVKN_DEBUG' in extra)
    hdrs.append(os.path.join(CSRC, 'vkn_chain.hip'))              # vkn_chain_h2.hip #includes it
    t_h = max(os.path.getmtime(h) for h in hdrs if os.path.exists(h))
    jobs, objs = [], []
    for s in SOURCES:
        src, obj = os.path.join(CSRC, s), os.path.join(objdir, s[:-4] + '.o')
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(t_h, os.path.getmtime(src)):
            jobs.append(['-O3', '-std=c++17', '-fPIC', *extra, '-c', src, '-o', obj])
    with ThreadPoolExecutor(max_workers=max(1, min(int(os.environ.get('VKN_BUILD_JOBS', '6')), os.cpu_count() or 1))) as ex:
        list(ex.map(lambda args: _hipcc(args, verbose), jobs))
    return objs


def _link(objs, out, verbose=False):
    _hipcc(['-shared', '-fPIC', *objs, '-o', out], verbose, 'hipcc link')


def build(force=False, verbose=False):
    """Compile csrc/*.hip for gfx950 into lib/libvkn.so (cross-compiles without a GPU): one object per source under lib/obj/,
    compiled in parallel, then one link."""
    os.makedirs(LIBDIR, exist_ok=True)
    if not force and not _stale():
        return LIBPATH
    _link(_compile_objects(os.path.join(LIBDIR, 'obj'), force=force, verbose=verbose), LIBPATH, verbose)
    return LIBPATH


def build_debug(force=False):
    """The same sources with -DVKN_DEBUG -> lib/libvkn_debug.so: the ONLY build that reads VKN_* environment knobs and contains
    the time-attribution kernel variants (tools/ only; never loaded by the package unless `use_debug()` is called first)."""
    os.makedirs(LIBDIR, exist_ok=True)
    if not force and not _stale(DEBUG_LIBPATH):
        return DEBUG_LIBPATH
    _link(_compile_objects(os.path.join(LIBDIR, 'obj_debug'), extra=('-DVKN_DEBUG',), force=force), DEBUG_LIBPATH)
    return DEBUG_LIBPATH


_LIB = None
_USE_DEBUG = False


def use_debug():
    """Measurement tools: load lib/libvkn_debug.so instead of the release library (must be called before the first op)."""
    global _USE_DEBUG
    if _LIB is not None:
        raise VknLibraryError('use_debug() must be called before the library is first used')
    _USE_DEBUG = True


def lib():
    """The loaded library (ctypes.CDLL) with the header's prototypes set.  Raises VknLibraryError when it is not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = DEBUG_LIBPATH if _USE_DEBUG else LIBPATH
    if not os.path.exists(path):
        raise VknLibraryError(f'{path} is missing — run `python -c "import __graft_entry__ as g; g.build()"` '
                              '(there is deliberately no CPU fallback)')
    L = ctypes.CDLL(path)
    for name, (result, params) in {**PROTOS, **TRACK_PROTOS, **TRACK_TRAIN_PROTOS, **GT_PROTOS, **DECODE_PROTOS}.items():
        fn = getattr(L, name)
        fn.restype = _ctype(*result, name, result=True)
        fn.argtypes = [POINTER_EXCEPTIONS.get((name, p)) or _ctype(base, depth, name) for p, base, depth in params]
    # header vs binary: structs are handed to the kernels verbatim, so a library built from another header means garbage pointers
    for name, mirror in {**MIRRORS, **TRACK_TRAIN_MIRRORS, **GT_MIRRORS}.items():
        probe = 'vkn_sizeof_' + re.sub(r'(?<!^)(?=[A-Z])', '_', name[3:]).lower()
        if probe not in PROTOS and probe not in TRACK_TRAIN_PROTOS and probe not in GT_PROTOS:
            raise VknLibraryError(f'include/vkn.h declares struct {name} without its size probe {probe}()')
        if getattr(L, probe)() != ctypes.sizeof(mirror):
            raise VknLibraryError(f'{path} does not match include/vkn.h: struct {name} is {getattr(L, probe)()} bytes in the library, '
                                  f'{ctypes.sizeof(mirror)} in the header')
    _LIB = L
    return L


def check(code):
    if code != 0:
        raise VknError(code, lib().vkn_strerror(code).decode())
