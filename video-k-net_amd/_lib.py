"""ctypes binding of libvkn.so, computed from its C ABI in the headers `ABI_HEADERS` under include/, + the hipcc build recipe.
`ABI` maps each header to what its own text declares (prototypes, structs, constants, ctypes mirrors); a header is read once, knowing
the headers it #includes, and no name may be declared twice.  `PROTOS`, `SYMBOLS`, `STRUCTS`, `MIRRORS` are include/vkn.h's part.
`EXTENSION_HEADERS` / `ABI_EXT` is a second such table behind the first: extension parts, read in the same pass and bound by the same loops.

The library is built IN-TREE (`video-k-net_amd/lib/libvkn.so`) so that it travels with the repo snapshot to the GPU
box; there is no CPU fallback: if the library is missing every op raises `VknLibraryError`.
"""
import collections
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIBDIR = os.path.join(HERE, 'lib')
LIBPATH = os.path.join(LIBDIR, 'libvkn.so')
SOURCES = ('vkn_gather.hip', 'vkn_update.hip', 'vkn_decode.hip', 'vkn_fused.hip', 'vkn_init.hip', 'vkn_panoptic.hip', 'vkn_merge.hip', 'vkn_assign.hip', 'vkn_assign_lr.hip', 'vkn_tracker.hip', 'vkn_loss.hip', 'vkn_chain.hip', 'vkn_chain_h2.hip', 'vkn_ksplit.hip', 'vkn_train.hip', 'vkn_wimage.hip', 'vkn_fpn.hip', 'vkn_optim.hip', 'vkn_tracktail.hip', 'vkn_trackloss.hip', 'vkn_gtprep.hip', 'vkn_segloss.hip', 'vkn_stq.hip', 'vkn_vpq.hip', 'vkn_fpn_bwd.hip', 'vkn_msda.hip', 'vkn_msda_bwd.hip', 'vkn_rle.hip', 'vkn_maskap.hip', 'vkn_instmask.hip', 'vkn_swin.hip', 'vkn_swin_bwd.hip', 'vkn_api.hip')
INCLUDE = os.path.join(os.path.dirname(HERE), 'include')
# The C ABI, one header per part, each behind the headers it #includes.  A new part is one more name here.
ABI_HEADERS = ('vkn.h', 'vkn_track.h', 'vkn_track_train.h', 'vkn_gt.h', 'vkn_decode.h')
# Extension parts: read, mirrored, bound and probed exactly as the headers above (after them, so they may #include any of those), but kept
# in their own table `ABI_EXT`, and their constants in their own records, not in `CONSTS`: `ABI` / `CONSTS` stay what ABI_HEADERS declare.
EXTENSION_HEADERS = ('vkn_seg_loss.h',)
# Metric parts: a third such table `ABI_METRIC` behind the two, on the same terms; its constants in their own record `STQ`.
METRIC_HEADERS = ('vkn_stq.h',)
# Windowed metric parts: a fourth such table `ABI_WINDOW_METRIC` behind the three, on the same terms; its constants in their own record `VPQ`.
WINDOW_METRIC_HEADERS = ('vkn_vpq.h',)
# Training parts: a fifth such table `ABI_TRAIN` behind the four, on the same terms; its constants in their own record `FPN_TRAIN`.
TRAIN_HEADERS = ('vkn_fpn_train.h',)
# Neck parts: a sixth such table `ABI_NECK` behind the five, on the same terms; its constants in their own record `MSDA`.
NECK_HEADERS = ('vkn_msda.h',)
# Neck training parts: a seventh such table `ABI_NECK_TRAIN` behind the six, on the same terms; its constants in their own record
# `MSDA_TRAIN`.  `_each`'s DEFAULT stays the six tables before it: the loops that bind go over `_bound`, the six and this one.
NECK_TRAIN_HEADERS = ('vkn_msda_train.h',)
# Result parts: an eighth such table `ABI_RESULT` behind the seven, on the same terms; its constants in their own record `RLE`.  `_bound`
# stays the seven tables before it; `_every` is the seven and this one.
RESULT_HEADERS = ('vkn_rle.h',)
# Instance metric parts: a ninth such table `ABI_INSTANCE_METRIC` behind the eight, on the same terms; its constants in their own record
# `MASKAP`.  `_every` stays the eight tables before it: the loops that bind go over `_all_bound`, the eight and this one.
INSTANCE_METRIC_HEADERS = ('vkn_maskap.h',)
# Instance result parts: a tenth such table `ABI_INSTANCE_RESULT` behind the nine, on the same terms; its constants in their own record
# `INSTMASK`.  `_all_bound` stays the nine tables before it: the loops that bind go over `_all_parts`, the nine and this one.
INSTANCE_RESULT_HEADERS = ('vkn_instmask.h',)
# Backbone parts: an eleventh such table `ABI_BACKBONE` behind the ten, on the same terms; its constants in their own record `SWIN`.
# `_all_parts` stays the ten tables before it: the loops that bind go over `_all_tables`, the ten and this one.
BACKBONE_HEADERS = ('vkn_swin.h',)
# Backbone training parts: a twelfth such table `ABI_BACKBONE_TRAIN` behind the eleven, on the same terms; its constants in their own record
# `WATTN_TRAIN`.  `_all_tables` stays the eleven tables before it: the loops that bind go over `_all_abi`, the eleven and this one.
BACKBONE_TRAIN_HEADERS = ('vkn_wattn_train.h',)


class VknLibraryError(RuntimeError):
    pass


class VknError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'libvkn error {code}: {msg}')
        self.code = code


# ---- the reader of include/*.h.  Everything here that restates the C ABI (prototypes, struct mirrors, constants) is computed from
#      the headers by it, once per process.  It knows exactly the C subset they are written in and refuses the rest.
_SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'unsigned int': ctypes.c_uint, 'size_t': ctypes.c_size_t,
            'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong}
_POINTEES = {'void', 'char', 'unsigned char', 'int64_t'}     # types the headers only ever point at
_DECLARATOR = re.compile(r'([\w\s]*?)\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[(\w+)\])?')
_COMMENT = re.compile(r'/\*.*?\*/|//[^\n]*', flags=re.S)


def _int(text, consts, where):
    """`64`, `1u`, `0x000600`, `(-3)`, `(VKN_A | VKN_B)` -> int"""
    total = 0
    for term in text.strip('() \t').split('|'):
        term = term.strip()
        if not (term in consts or re.fullmatch(r'-?\d+|\d+u|0x[0-9a-fA-F]+', term)):
            raise VknLibraryError(f'{where}: {text.strip()!r} is not an integer this binding can read')
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
            raise VknLibraryError(f'{where}: cannot read the declaration {" ".join(decl.split())!r}')
        out.append((m.group(3), base, m.group(2).count('*'), m.group(4) and _int(m.group(4), consts, where)))
    return out


def read_header(text, known_structs=(), known_consts=(), where='include/vkn.h'):
    """(prototypes, structs, constants) that a header written in vkn.h's C subset declares itself:
    prototypes {function: ((base type, pointer depth) of the result, [(parameter, base type, pointer depth)])},
    structs {name: [(field, base type, pointer depth, array length or None)]}, constants {VKN_*: int}; all in the header's order.
    `known_structs` (names) and `known_consts` ({VKN_*: int}) are what the headers it #includes declare; `where` names it in errors.
    Raises VknLibraryError naming the declaration it cannot read."""
    text = _COMMENT.sub(' ', text)
    consts, structs, protos, known, values = {}, {}, {}, set(_SCALARS) | _POINTEES | set(known_structs), dict(known_consts)
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(VKN_\w+)(.*)$', text, flags=re.M):
        if value.strip():                                               # (the include guard has no value)
            consts[name] = values[name] = _int(value, values, f'{where}: {name}')
    text = re.sub(r'#ifdef __cplusplus.*?#endif', '', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)

    def struct(m):
        structs[m.group(2)] = [f for d in m.group(1).split(';') if d.strip() for f in _declaration(d, known, values, f'{where}: {m.group(2)}')]
        known.add(m.group(2))
        return ''
    text = re.sub(r'typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;', struct, text)
    for decl in filter(None, (' '.join(d.split()) for d in text.split(';'))):
        m = re.fullmatch(r'([\w\s\*]+?)\b(vkn_\w+)\s*\(([^()]*)\)', decl)
        if not m:
            raise VknLibraryError(f'{where}: cannot read the declaration {decl[:120]!r}')
        at = f'{where}: {m.group(2)}'
        (_, rbase, rdepth, _), = _declaration(m.group(1) + ' result', known, values, at)
        params = [] if m.group(3).strip() == 'void' else [q for p in m.group(3).split(',') for q in _declaration(p, known, values, at)]
        if any(length is not None for *_, length in params):
            raise VknLibraryError(f'{at}: array parameters are not supported')
        protos[m.group(2)] = ((rbase, rdepth), [q[:3] for q in params])
    return protos, structs, consts


AbiHeader = collections.namedtuple('AbiHeader', 'path protos symbols structs consts mirrors')      # what ONE header's own text declares


def read_abi(include_dir, names):
    """{header name: AbiHeader} of the headers `names` under `include_dir`, each read once, in order.  A header is read knowing the
    structs and constants of the headers its own `#include "..."` lines name, transitively (`<...>` includes are the C library's and
    are ignored).  Raises VknLibraryError when a header includes a file that is not earlier in `names`, and when two headers declare
    the same function, struct or constant.  `mirrors` is left empty: building the ctypes classes is the caller's step."""
    abi, deps, owner = {}, {}, {}
    for name in names:
        with open(os.path.join(include_dir, name)) as f:
            text = f.read()
        deps[name] = []
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', _COMMENT.sub(' ', text), flags=re.M):
            if inc not in abi:
                raise VknLibraryError(f'include/{name} includes "{inc}", which is not among the headers listed before it: {tuple(abi)}')
            deps[name] += [d for d in deps[inc] + [inc] if d not in deps[name]]
        protos, structs, consts = read_header(text, [s for d in deps[name] for s in abi[d].structs],
                                              {k: v for d in deps[name] for k, v in abi[d].consts.items()}, f'include/{name}')
        for declared in (*protos, *structs, *consts):
            if owner.setdefault(declared, name) != name:
                raise VknLibraryError(f'{declared} is declared twice: by include/{owner[declared]} and by include/{name}')
        abi[name] = AbiHeader(f.name, protos, tuple(protos), structs, consts, {})
    return abi


def _each(field, tables=None):
    """[(header, name, value)] of one field of every header's record — `ABI`'s, then `ABI_EXT`'s, `ABI_METRIC`'s, `ABI_WINDOW_METRIC`'s, `ABI_TRAIN`'s, `ABI_NECK`'s — in the headers' order"""
    return [(h, k, v) for t in (tables or (ABI, ABI_EXT, ABI_METRIC, ABI_WINDOW_METRIC, ABI_TRAIN, ABI_NECK)) for h, hdr in t.items() for k, v in getattr(hdr, field).items()]


def _bound(field):
    """`_each` over every table that is bound: its default six, then `ABI_NECK_TRAIN`"""
    return _each(field) + _each(field, (ABI_NECK_TRAIN,))


def _every(field):
    """`_bound`'s seven tables, then `ABI_RESULT`"""
    return _bound(field) + _each(field, (ABI_RESULT,))


def _all_bound(field):
    """`_every`'s eight tables, then `ABI_INSTANCE_METRIC`: the nine tables before `ABI_INSTANCE_RESULT`"""
    return _every(field) + _each(field, (ABI_INSTANCE_METRIC,))


def _all_parts(field):
    """`_all_bound`'s nine tables, then `ABI_INSTANCE_RESULT`: the ten tables before `ABI_BACKBONE`"""
    return _all_bound(field) + _each(field, (ABI_INSTANCE_RESULT,))


def _all_tables(field):
    """`_all_parts`'s ten tables, then `ABI_BACKBONE`: the eleven tables before `ABI_BACKBONE_TRAIN`"""
    return _all_parts(field) + _each(field, (ABI_BACKBONE,))


def _all_abi(field):
    """`_all_tables`'s eleven tables, then `ABI_BACKBONE_TRAIN`: every table that is bound"""
    return _all_tables(field) + _each(field, (ABI_BACKBONE_TRAIN,))


_EVERY_HEADER = ABI_HEADERS + EXTENSION_HEADERS + METRIC_HEADERS + WINDOW_METRIC_HEADERS + TRAIN_HEADERS + NECK_HEADERS + NECK_TRAIN_HEADERS + RESULT_HEADERS + INSTANCE_METRIC_HEADERS + INSTANCE_RESULT_HEADERS + BACKBONE_HEADERS + BACKBONE_TRAIN_HEADERS
_ALL = read_abi(INCLUDE, _EVERY_HEADER)          # ONE reading: includes resolve, a name declared twice is an error
ABI = {h: _ALL[h] for h in ABI_HEADERS}
ABI_EXT = {h: _ALL[h] for h in EXTENSION_HEADERS}
ABI_METRIC = {h: _ALL[h] for h in METRIC_HEADERS}
ABI_WINDOW_METRIC = {h: _ALL[h] for h in WINDOW_METRIC_HEADERS}
ABI_TRAIN = {h: _ALL[h] for h in TRAIN_HEADERS}
ABI_NECK = {h: _ALL[h] for h in NECK_HEADERS}
ABI_NECK_TRAIN = {h: _ALL[h] for h in NECK_TRAIN_HEADERS}
ABI_RESULT = {h: _ALL[h] for h in RESULT_HEADERS}
ABI_INSTANCE_METRIC = {h: _ALL[h] for h in INSTANCE_METRIC_HEADERS}
ABI_INSTANCE_RESULT = {h: _ALL[h] for h in INSTANCE_RESULT_HEADERS}
ABI_BACKBONE = {h: _ALL[h] for h in BACKBONE_HEADERS}
ABI_BACKBONE_TRAIN = {h: _ALL[h] for h in BACKBONE_TRAIN_HEADERS}
HEADER, PROTOS, SYMBOLS, STRUCTS, MIRRORS = (getattr(ABI['vkn.h'], k) for k in ('path', 'protos', 'symbols', 'structs', 'mirrors'))
CONSTS = {k: v for _, k, v in _each('consts', (ABI,))}      # every ABI header's constants: no name is declared twice
SEG = ABI_EXT['vkn_seg_loss.h'].consts              # an extension's constants stay in its own record
STQ = ABI_METRIC['vkn_stq.h'].consts                # ... and so do a metric part's
VPQ = ABI_WINDOW_METRIC['vkn_vpq.h'].consts         # ... and a windowed metric part's
FPN_TRAIN = ABI_TRAIN['vkn_fpn_train.h'].consts     # ... and a training part's
MSDA = ABI_NECK['vkn_msda.h'].consts                # ... and a neck part's
MSDA_TRAIN = ABI_NECK_TRAIN['vkn_msda_train.h'].consts      # ... and a neck training part's
RLE = ABI_RESULT['vkn_rle.h'].consts                # ... and a result part's
MASKAP = ABI_INSTANCE_METRIC['vkn_maskap.h'].consts   # ... and an instance metric part's
INSTMASK = ABI_INSTANCE_RESULT['vkn_instmask.h'].consts   # ... and an instance result part's
SWIN = ABI_BACKBONE['vkn_swin.h'].consts                  # ... and a backbone part's
WATTN_TRAIN = ABI_BACKBONE_TRAIN['vkn_wattn_train.h'].consts      # ... and a backbone training part's
GT_MAX_IMAGES = CONSTS['VKN_GT_MAX_IMAGES']
GT_MAX_CLASSES = CONSTS['VKN_GT_MAX_CLASSES']
GT_MAX_IDS = CONSTS['VKN_GT_MAX_IDS']
TRACK_LOSS_MAX_ROWS = CONSTS['VKN_TRACK_LOSS_MAX_ROWS']
TRACK_MAX_K = CONSTS['VKN_TRACK_MAX_K']
MAX_FCS = CONSTS['VKN_MAX_FCS']
SPLIT_MAX_ITEMS = CONSTS['VKN_SPLIT_MAX_ITEMS']
DW_MAX_ITEMS = CONSTS['VKN_DW_MAX_ITEMS']
ADAMW_GROUP_ROW = CONSTS['VKN_ADAMW_GROUP_ROW']     # lr, weight_decay, beta1, beta2, eps (fp64)
_MIRROR = {}                                # struct name -> ctypes.Structure, of every header: where _ctype looks a struct up


def _ctype(base, depth, where, result=False):
    """Scalars by value; `const char*` results as bytes; a pointer to a mirrored struct typed; every other pointer (device memory, for the
    most part) travels as an integer."""
    if depth == 0 and base in _SCALARS:
        return _SCALARS[base]
    if depth == 1 and base == 'char' and result:
        return ctypes.c_char_p
    if depth == 1 and base in _MIRROR:
        return ctypes.POINTER(_MIRROR[base])
    if depth == 0:
        raise VknLibraryError(f'{where}: {base!r} by value has no ctypes counterpart here')
    return ctypes.c_void_p


for _h, _name, _fields in _all_abi('structs'):
    _at = f'include/{_h}: {_name}'
    _ALL[_h].mirrors[_name] = _MIRROR[_name] = type(_name, (ctypes.Structure,), {
        '__doc__': f'Mirror of {_at} (device pointers as integers).',
        '_fields_': [(f, _ctype(b, d, _at) * n if n else _ctype(b, d, _at)) for f, b, d, n in _fields]})
# importable by name: VknDims, VknStageWeights, VknSplitItem, VknDwItem, VknUpdatorNorms, VknUpdatorNormGrads, VknPanopticCfg, VknAssignCfg,
# VknAssignProblem, VknLsapProblem, VknTailImage, VknTailCfg, VknAdamwItem, VknTrackerCfg, VknTrackLossCfg, VknGtImage, VknSegImage, VknStqCfg, VknVpqCfg, VknMaskApCfg, VknInstMaskCfg
globals().update(_MIRROR)

# The pointer parameters that do NOT follow _ctype's rule: (function, parameter) -> ctypes type.
POINTER_EXCEPTIONS = {
    ('vkn_adamw_flat_f32', 'items'): ctypes.c_void_p,       # the VknAdamwItem array lives in DEVICE memory: callers pass tensor.data_ptr()
    ('vkn_sum_n_f32', 'srcs'): ctypes.POINTER(ctypes.c_void_p),                   # a HOST array of device pointers, (c_void_p * n)(...)
    ('vkn_qd_tracker_state_layout', 'offsets12'): ctypes.POINTER(ctypes.c_size_t),  # a HOST array the call fills, (c_size_t * 12)()
    ('vkn_stq_state_layout', 'offsets8'): ctypes.POINTER(ctypes.c_size_t),          # likewise, (c_size_t * 8)()
    ('vkn_vpq_state_layout', 'offsets4'): ctypes.POINTER(ctypes.c_size_t),          # likewise, (c_size_t * 4)()
    ('vkn_mask_ap_state_layout', 'offsets3'): ctypes.POINTER(ctypes.c_size_t),      # likewise, (c_size_t * 3)()
    ('vkn_msda_sample_f32', 'shapes'): ctypes.POINTER(ctypes.c_int),                # a HOST array of L (H, W) pairs, (c_int * 2L)(...)
    ('vkn_msda_bwd_workspace_bytes', 'shapes'): ctypes.POINTER(ctypes.c_int),       # likewise
    ('vkn_msda_sample_bwd_f32', 'shapes'): ctypes.POINTER(ctypes.c_int),            # likewise
}
for _fn, _p in set(POINTER_EXCEPTIONS) - {(fn, q[0]) for _, fn, (_, params) in _all_abi('protos') for q in params}:
    raise VknLibraryError(f'POINTER_EXCEPTIONS names {_fn}({_p}), which none of the headers {_EVERY_HEADER} declares')

DEBUG_LIBPATH = os.path.join(LIBDIR, 'libvkn_debug.so')


def _hipcc(args, verbose=False, what='hipcc'):
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', *args]
    if verbose:
        print(' '.join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise VknLibraryError(f'{what} failed:\n' + r.stdout + r.stderr)


def _shared_deps(debug):
    """What every object depends on besides csrc/: the public headers and, in the debug build, the kernel variants it #includes."""
    exp = os.path.join(os.path.dirname(HERE), 'tools', 'experiments')
    return [h.path for h in _ALL.values()] + ([os.path.join(exp, f) for f in os.listdir(exp)] if debug and os.path.isdir(exp) else [])


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
    """The loaded library (ctypes.CDLL) with the headers' prototypes set.  Raises VknLibraryError when it is not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = DEBUG_LIBPATH if _USE_DEBUG else LIBPATH
    if not os.path.exists(path):
        raise VknLibraryError(f'{path} is missing — run `python -c "import __graft_entry__ as g; g.build()"` '
                              '(there is deliberately no CPU fallback)')
    L = ctypes.CDLL(path)
    for h, name, (result, params) in _all_abi('protos'):
        fn, at = getattr(L, name), f'include/{h}: {name}'
        fn.restype = _ctype(*result, at, result=True)
        fn.argtypes = [POINTER_EXCEPTIONS.get((name, p)) or _ctype(base, depth, at) for p, base, depth in params]
    # header vs binary: structs are handed to the kernels verbatim, so a library built from another header means garbage pointers
    for h, name, mirror in _all_abi('mirrors'):
        probe = 'vkn_sizeof_' + re.sub(r'(?<!^)(?=[A-Z])', '_', name[3:]).lower()
        if not any(probe in hdr.protos for hdr in _ALL.values()):        # any header may declare a struct's size probe
            raise VknLibraryError(f'include/{h} declares struct {name} without its size probe {probe}()')
        if getattr(L, probe)() != ctypes.sizeof(mirror):
            raise VknLibraryError(f'{path} does not match include/{h}: struct {name} is {getattr(L, probe)()} bytes in the library, '
                                  f'{ctypes.sizeof(mirror)} in the header')
    _LIB = L
    return L


def check(code):
    if code != 0:
        raise VknError(code, lib().vkn_strerror(code).decode())
