"""Call signatures: for every class on the path that the reference defines and this package mirrors, every method the reference's
class defines itself must exist here with the reference's parameter names in the reference's order (extra parameters here must
have defaults) — what "same names, argument meaning" of a drop-in means mechanically.  The reference's side is stored data
(tests/golden/reference_api_surface.json: its classes imported UNMODIFIED through the plumbing stand-ins of oracle/standins by
oracle/gen_golden_api.py, which also holds the list of class pairs)."""
import inspect
import json
import os

from oracle.gen_golden_api import PAIRS      # reference class -> class here

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_api_surface.json')

# methods of the reference this package deliberately does not carry (reason beside each)
NOT_BUILT = {
    'VideoKernelIterHead': {'merge_stuff_thing_stuff_first'},      # dead code in the reference: nothing calls it
    # the memo update (births, momentum embeddings, velocities, backdrops, expiry) happens INSIDE the device match kernel; the method exists
    # and raises NotImplementedError with that explanation — listed here so that the surface test does not count it as carried
    'QuasiDenseEmbedTracker': {'update_memo'},
}


def _reference_surface():
    with open(FIXTURE) as f:
        surf = json.load(f)
    assert sorted(surf) == sorted(PAIRS), 'tests/golden/reference_api_surface.json does not cover the class pairs: run oracle/gen_golden_api.py'
    return surf


def test_methods_and_parameter_names_follow_the_reference(vkn):
    surf = _reference_surface()
    problems = []
    checked = 0
    for key, here in sorted(PAIRS.items()):
        ref = surf[key]
        if '__error__' in ref:
            problems.append(f'{key}: reference class not importable: {ref["__error__"]}')
            continue
        cls = vkn
        for part in here.split('.'):
            cls = getattr(cls, part, None) if cls is not None else None
        cls = cls or vkn.HEADS.get(here)
        assert cls is not None, here
        for name, rparams in sorted(ref.items()):
            if name in NOT_BUILT.get(here, ()):
                continue
            fn = getattr(cls, name, None)
            if fn is None:
                problems.append(f'{here}.{name}: missing')
                continue
            mine = list(inspect.signature(fn).parameters.values())
            if mine and mine[0].name == 'self' and not (rparams and rparams[0][0] == 'self'):
                mine = mine[1:]
            var_kw = any(p.kind.name == 'VAR_KEYWORD' for p in mine)
            var_pos = any(p.kind.name == 'VAR_POSITIONAL' for p in mine)
            names = [p.name for p in mine if p.kind.name not in ('VAR_KEYWORD', 'VAR_POSITIONAL')]
            rnames = [p[0] for p in rparams if p[2] not in ('VAR_KEYWORD', 'VAR_POSITIONAL')]
            for i, rn in enumerate(rnames):
                if i < len(names) and names[i] == rn:
                    continue
                if rn in names and rparams[i][1]:        # a defaulted parameter of the reference, present here by name (keyword use)
                    continue
                if (var_kw and rparams[i][1]) or (var_pos and not rparams[i][1] and i >= len(names)):
                    continue
                problems.append(f'{here}.{name}: reference parameter {i} `{rn}` vs here {names}')
                break
            extra = [p for p in mine if p.name not in rnames and p.kind.name not in ('VAR_KEYWORD', 'VAR_POSITIONAL')
                     and p.default is inspect._empty]
            if extra:
                problems.append(f'{here}.{name}: extra required parameters {[p.name for p in extra]}')
            checked += 1
    assert not problems, '\n'.join(problems)
    assert checked > 60
