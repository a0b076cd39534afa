"""What `STQMeter` and `VPQMeter` share: one device state per sequence, in order of first appearance, and its status word."""
import numpy as np
import torch

from . import _lib


class MapMeter:
    """A subclass sets `_BITS` ((constant name, text) per status bit), `_CONSTS` (its header's constants), `_new_state` (`ops.*_state`)
    and, before the first update, `self._cfg`."""

    def __init__(self, device):
        self.device = torch.device(device if device is not None else 'cuda')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._states = {}                                   # sequence id -> device state, in order of first appearance

    def _state(self, sequence_id):
        state = self._states.get(sequence_id)
        if state is None:
            state = self._states[sequence_id] = self._new_state(self._cfg, self.device)
        return state

    def reset_states(self):
        self._states = {}

    @classmethod
    def _status_text(cls, status):
        return '; '.join(text for name, text in cls._BITS if status & cls._CONSTS[name])

    def _raise_on(self, sequence_id, status):
        if status:
            raise _lib.VknError(_lib.CONSTS['VKN_E_RANGE'], f'{type(self).__name__}: sequence {sequence_id!r}: status {status:#x}: {self._status_text(status)}')

    def check_status(self):
        """Raises VknError when any sequence's status word is set (reads 4 bytes per sequence: a synchronisation)."""
        for sid, state in self._states.items():
            self._raise_on(sid, int(state[0:4].cpu().numpy().view(np.uint32)[0]))
