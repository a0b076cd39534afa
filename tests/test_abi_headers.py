"""CPU: the C ABI of libvkn, header by header.  `_lib.read_abi` reads every header of `_lib.ABI_HEADERS` once, behind the headers it
#includes, into `_lib.ABI`; what each header declares is pinned here, written out, and judged by readers other than `_lib`'s own: a
regex for the argument lists, a C compiler for the struct layouts and for the headers themselves, the built library for the exports."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('vkn.h', 'vkn_track.h', 'vkn_track_train.h', 'vkn_gt.h', 'vkn_decode.h')
COUNTS = {'vkn.h': 111, 'vkn_track.h': 5, 'vkn_track_train.h': 4, 'vkn_gt.h': 4, 'vkn_decode.h': 3}
SYMBOLS = {         # the exact symbol set of every header but vkn.h (whose 111 names test_host_logic.py reads from its text)
    'vkn_track.h': {'vkn_track_boxes_workspace_bytes', 'vkn_track_boxes_f32', 'vkn_track_maps_workspace_bytes', 'vkn_track_maps_i32',
                    'vkn_qd_tracker_match_dev_f32'},
    'vkn_track_train.h': {'vkn_sizeof_track_loss_cfg', 'vkn_track_loss_workspace_bytes', 'vkn_track_loss_fwd_f32', 'vkn_track_loss_bwd_f32'},
    'vkn_gt.h': {'vkn_sizeof_gt_image', 'vkn_gt_classes', 'vkn_gt_bank_fill_f32', 'vkn_gt_match_indices'},
    'vkn_decode.h': {'vkn_mask_decode_planes_wg_f32', 'vkn_mask_decode_planes_wg_x', 'vkn_decode_px_per_wg'},
}
ARGUMENTS = {'vkn_track_boxes_f32': 21, 'vkn_track_maps_i32': 18, 'vkn_qd_tracker_match_dev_f32': 16, 'vkn_track_loss_fwd_f32': 18,
             'vkn_track_loss_bwd_f32': 12, 'vkn_gt_classes': 12, 'vkn_gt_bank_fill_f32': 9, 'vkn_gt_match_indices': 8,
             'vkn_mask_decode_planes_wg_f32': 11, 'vkn_mask_decode_planes_wg_x': 12, 'vkn_decode_px_per_wg': 3}
STRUCTS = {'vkn.h': 14, 'vkn_track.h': [], 'vkn_track_train.h': ['VknTrackLossCfg'], 'vkn_gt.h': ['VknGtImage'], 'vkn_decode.h': []}
MAINS = {           # a C99 translation unit per header: it includes that header alone and uses what the header adds
    'vkn.h': 'int main(void) { VknDims d; VknStageWeights w; VknSplitItem a; VknDwItem b; VknUpdatorNorms c; VknUpdatorNormGrads g;\n'
             '  (void)d; (void)w; (void)a; (void)b; (void)c; (void)g; return vkn_version() == 0; }\n',
    'vkn_track.h': 'int main(void) { return VKN_TRACK_MAX_K > 0 ? 0 : 1; }\n',
    'vkn_track_train.h': 'int main(void) { VknTrackLossCfg c; c.has_aux = VKN_TRACK_LOSS_MAX_ROWS; return c.has_aux > VKN_TRACK_MAX_K ? 1 : 0; }\n',
    'vkn_gt.h': 'int main(void) { VknGtImage im; im.G = VKN_GT_MAX_IDS; return im.G > VKN_GT_MAX_CLASSES * VKN_GT_MAX_IMAGES ? 1 : 0; }\n',
    'vkn_decode.h': 'int main(void) { return vkn_decode_px_per_wg(1, 512, 0) > 0 ? 0 : 1; }\n',
}


def _compile(std, src):
    """Syntax-check one C file against the repository root with every warning an error: by the host C compiler, or, where there is
    none, by the compiler the build needs anyway, in C mode, host side only."""
    cc = shutil.which('gcc') or shutil.which('cc')
    cmd = [cc] if cc is not None else [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c']
    r = subprocess.run(cmd + [f'-std={std}', '-Wall', '-Wextra', '-Werror', '-fsyntax-only', '-I', ROOT, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_table_is_the_five_headers(vkn):
    lib = vkn._lib
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI)
    assert {h: len(lib.ABI[h].symbols) for h in HEADERS} == COUNTS
    for a, b in itertools.combinations(HEADERS, 2):
        assert not set(lib.ABI[a].symbols) & set(lib.ABI[b].symbols), (a, b)
    for h in HEADERS:
        assert lib.ABI[h].path == os.path.join(ROOT, 'include', h) and lib.ABI[h].symbols == tuple(lib.ABI[h].protos)
    vkn_h = lib.ABI['vkn.h']        # "what vkn.h declares" keeps its plain names
    assert (lib.HEADER, lib.PROTOS, lib.SYMBOLS, lib.STRUCTS, lib.MIRRORS) == (vkn_h.path, vkn_h.protos, vkn_h.symbols, vkn_h.structs, vkn_h.mirrors)
    assert lib.PROTOS is vkn_h.protos and lib.MIRRORS is vkn_h.mirrors
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()}
    assert sum(len(lib.ABI[h].consts) for h in HEADERS) == len(lib.CONSTS)


@pytest.mark.parametrize('header', HEADERS)
def test_header_is_exported_with_its_own_argument_lists(vkn, header):
    """The binding of a header is that header: the symbol set pinned above, exported by the raw library, and for every declared function
    the argument count that this test's own reading of the header text gives (a regex, not `_lib.read_header`)."""
    lib = vkn._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    names = [name for name, _ in declared]
    assert len(names) == len(set(names)) == COUNTS[header]
    assert set(names) == set(lib.ABI[header].symbols) == set(lib.ABI[header].protos) == SYMBOLS.get(header, set(names))
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert getattr(raw, name) is not None
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype in (ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p), name
        assert len(fn.argtypes) == (0 if params.strip() == 'void' else params.count(',') + 1), name
        assert len(fn.argtypes) == ARGUMENTS.get(name, len(fn.argtypes)), name


def test_pinned_argument_and_result_types(vkn):
    lib = vkn._lib
    L = lib.lib()
    assert set(ARGUMENTS) <= set().union(*SYMBOLS.values())
    assert {name: len(getattr(L, name).argtypes) for name in ARGUMENTS} == ARGUMENTS
    assert L.vkn_qd_tracker_match_dev_f32.argtypes[0]._type_ is lib.VknTrackerCfg
    assert L.vkn_track_loss_fwd_f32.argtypes[0]._type_ is lib.VknTrackLossCfg
    for fn in (L.vkn_gt_classes, L.vkn_gt_bank_fill_f32):
        assert fn.argtypes[0]._type_ is lib.VknGtImage
    assert L.vkn_track_boxes_workspace_bytes.restype is ctypes.c_size_t and L.vkn_track_loss_workspace_bytes.restype is ctypes.c_size_t


def test_struct_ownership_fields_and_sizes(vkn):
    lib = vkn._lib
    L = lib.lib()
    assert len(lib.ABI['vkn.h'].structs) == len(lib.MIRRORS) == STRUCTS['vkn.h'] == 14
    for h in HEADERS[1:]:
        assert list(lib.ABI[h].structs) == list(lib.ABI[h].mirrors) == STRUCTS[h], h
    assert 'VknTrackLossCfg' not in lib.MIRRORS and 'VknGtImage' not in lib.MIRRORS
    for h in HEADERS:
        assert all(getattr(lib, n) is m for n, m in lib.ABI[h].mirrors.items())         # importable by name
    fields = {n: [f for f, *_ in s] for h in HEADERS for n, s in lib.ABI[h].structs.items()}
    assert fields['VknTrackLossCfg'] == ['softmax_temp', 'has_aux', 'w_track', 'w_aux', 'neg_pos_ub', 'pos_margin', 'neg_margin']
    assert fields['VknGtImage'] == ['masks', 'sem', 'classes', 'G', 'Hm', 'Wm', 'valid_h', 'valid_w', 'n_sem', 'row0', 'sem_row0']
    assert all([f for f, _ in getattr(lib, n)._fields_] == fs for n, fs in fields.items())
    assert L.vkn_sizeof_track_loss_cfg() == ctypes.sizeof(lib.VknTrackLossCfg) == 28
    assert L.vkn_sizeof_gt_image() == ctypes.sizeof(lib.VknGtImage) == 56


def test_constants_and_sources(vkn):
    lib = vkn._lib
    assert (lib.GT_MAX_IMAGES, lib.GT_MAX_CLASSES, lib.GT_MAX_IDS) == (64, 256, 1024)
    assert lib.TRACK_LOSS_MAX_ROWS == 128
    assert (lib.CONSTS['VKN_FLAG_LINK_RESERVE'], lib.CONSTS['VKN_FLAG_LINK_NO_RESERVE']) == (262144, 524288)
    assert 'vkn_gtprep.hip' in lib.SOURCES


@pytest.mark.parametrize('header', HEADERS)
def test_header_is_c99_on_its_own(header, tmp_path):
    """Every header is the drop-in boundary of its part: a C99 translation unit that includes it alone (and uses what it adds) must
    compile: no C++-isms, no torch / HIP types in the signatures, nothing that another header would have had to declare first."""
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{header}"\n' + MAINS[header])
    _compile('c99', src)


@pytest.mark.parametrize('header', HEADERS)
def test_struct_mirrors_have_the_layout_a_c_compiler_gives_the_header(vkn, header, tmp_path):
    """The ctypes mirrors are computed from the headers by `_lib.read_header`; a C compiler, not that reader, is the judge of the result:
    offset and size of every field and the size of every struct, as `_Static_assert`s in a translation unit that includes only the
    header that declares them (C11 for `_Static_assert`, this generated file only).  Catches what the library's `vkn_sizeof_*` probes
    cannot: two fields of one size swapped, a float read as an int."""
    mirrors = vkn._lib.ABI[header].mirrors
    lines = ['#include <stddef.h>', f'#include "include/{header}"']
    for name, m in mirrors.items():
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(m)}, "sizeof {name}");')
        for field, _ in m._fields_:
            f = getattr(m, field)
            lines.append(f'_Static_assert(offsetof({name}, {field}) == {f.offset}, "offsetof {name}.{field}");')
            lines.append(f'_Static_assert(sizeof((({name}*)0)->{field}) == {f.size}, "sizeof {name}.{field}");')
    assert len(lines) == 2 + len(mirrors) + 2 * sum(len(m._fields_) for m in mirrors.values())
    if header == 'vkn.h':
        assert len(mirrors) == 14 and len(lines) > 2 + 14 + 2 * 150
    elif STRUCTS[header]:
        assert len(lines) == 2 + 1 + 2 * {'VknTrackLossCfg': 7, 'VknGtImage': 11}[STRUCTS[header][0]]
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    _compile('c11', src)


# ---------------------------------------------------------------------------------------------------- the reader, on headers written here
BASE = ('#ifndef VKN_BASE_H\n#define VKN_BASE_H\n#include <stddef.h>\n#define VKN_N 4\n'
        'typedef struct VknCfg { int n; float w[VKN_N]; } VknCfg;\nint vkn_base(const VknCfg* cfg, void* stream);\n#endif\n')
SAT = ('#ifndef VKN_SAT_H\n#define VKN_SAT_H\n#include "base.h"\n#define VKN_M (VKN_N | 8)\n'
       'typedef struct VknSat { const float* rows[VKN_M]; } VknSat;\nsize_t vkn_sat(const VknCfg* cfg, const VknSat* s);\n#endif\n')


def _write(tmp_path, **texts):
    for name, text in texts.items():
        (tmp_path / (name + '.h')).write_text(text)
    return str(tmp_path)


def test_a_header_resolves_what_the_headers_it_includes_declare(vkn, tmp_path):
    """Each record holds what its own header's text declares; structs and constants of the included headers are known to the reader,
    transitively, and are not restated."""
    third = '#include "sat.h"\nint vkn_third(const VknCfg* cfg, const VknSat* s);\n'          # VknCfg reaches it through sat.h
    abi = vkn._lib.read_abi(_write(tmp_path, base=BASE, sat=SAT, third=third), ('base.h', 'sat.h', 'third.h'))
    assert list(abi) == ['base.h', 'sat.h', 'third.h'] and abi['sat.h'].path == str(tmp_path / 'sat.h')
    assert abi['base.h'].consts == dict(VKN_N=4) and abi['sat.h'].consts == dict(VKN_M=12) and abi['third.h'].consts == {}
    assert list(abi['base.h'].structs) == ['VknCfg'] and abi['third.h'].structs == {}
    assert abi['sat.h'].structs == dict(VknSat=[('rows', 'float', 1, 12)])
    assert abi['sat.h'].protos == dict(vkn_sat=(('size_t', 0), [('cfg', 'VknCfg', 1), ('s', 'VknSat', 1)]))
    assert abi['third.h'].symbols == ('vkn_third',) and abi['third.h'].protos['vkn_third'][1][1] == ('s', 'VknSat', 1)
    # the shipped case: vkn_track.h takes `const VknTrackerCfg*` from vkn.h, and on its own does not know it
    lib = vkn._lib
    assert ('cfg', 'VknTrackerCfg', 1) in lib.ABI['vkn_track.h'].protos['vkn_qd_tracker_match_dev_f32'][1]
    assert 'VknTrackerCfg' in lib.ABI['vkn.h'].structs and not lib.ABI['vkn_track.h'].structs
    with pytest.raises(vkn.VknLibraryError) as e:
        lib.read_header(open(lib.ABI['vkn_track.h'].path).read())
    assert 'VknTrackerCfg' in str(e.value)


@pytest.mark.parametrize('names,missing', [(('sat.h', 'base.h'), 'base.h'), (('sat.h',), 'base.h'), (('base.h', 'sat.h'), 'other.h')])
def test_an_include_that_is_not_earlier_in_the_list_is_refused(vkn, tmp_path, names, missing):
    sat = SAT if missing == 'base.h' else SAT.replace('#include "base.h"', '#include "base.h"\n#include "other.h"')
    with pytest.raises(vkn.VknLibraryError) as e:
        vkn._lib.read_abi(_write(tmp_path, base=BASE, sat=sat, other=''), names)
    assert 'sat.h' in str(e.value) and f'"{missing}"' in str(e.value)


@pytest.mark.parametrize('twice,line', [('vkn_base', 'int vkn_base(int n);'), ('VknCfg', 'typedef struct VknCfg { int n; } VknCfg;'),
                                        ('VKN_N', '#define VKN_N 4')])
def test_a_name_declared_by_two_headers_is_refused(vkn, tmp_path, twice, line):
    """whether or not the second header includes the first"""
    for second in (SAT.replace('#define VKN_M', line + '\n#define VKN_M'), line + '\n'):
        with pytest.raises(vkn.VknLibraryError) as e:
            vkn._lib.read_abi(_write(tmp_path, base=BASE, sat=second), ('base.h', 'sat.h'))
        assert re.search(rf'\b{twice}\b', str(e.value)) and 'base.h' in str(e.value) and 'sat.h' in str(e.value), str(e.value)


@pytest.mark.parametrize('bad,named', [('int vkn_odd(const VknCfg* cfg, half_t scale);', 'vkn_odd'), ('typedef struct VknU { wchar_t* s; } VknU;', 'VknU'),
                                       ('#define VKN_E (1 << 4)', 'VKN_E'), ('int vkn_arr(float x[VKN_N]);', 'vkn_arr'), ('int other(void);', 'other')])
def test_an_unreadable_declaration_is_reported_under_its_own_header(vkn, tmp_path, bad, named):
    with pytest.raises(vkn.VknLibraryError) as e:
        vkn._lib.read_abi(_write(tmp_path, base=BASE, sat=SAT.replace('#endif', bad + '\n#endif')), ('base.h', 'sat.h'))
    assert named in str(e.value) and 'sat.h' in str(e.value) and 'vkn.h' not in str(e.value) and 'base.h' not in str(e.value), str(e.value)
