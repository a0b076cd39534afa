"""`TrackTrainTail` — the training counterpart of `TrackTail`: the end of the "Tracking Part" of `forward_train`
(knet/video/knet_quansi_dense_embed_fc_joint_train.py:425-460) on the device, without a host synchronisation.

    object_feats_track, ref_obj_feats -> [:num_proposals] -> embed (embed_fcs + fc_embed) -> track_head   (torch, under autograd, ALL rows)
                                      -> fused match / targets / losses + their backward                  (csrc/vkn_trackloss.hip)

The reference gathers the positive rows first (`pos_inds`, :440-452: a `nonzero` behind the sampler) and runs the track head on them;
the embedding layers and the head are row-wise, so running them on all `num_proposals` rows gives the same rows, and the kernel
compacts the positives itself from the assigner's `gt_inds`.  The class owns no parameters.
"""
import torch

from . import _lib


class TrackTrainTail:
    """Built from the detector's `num_proposals`, its `track_head` (`QuasiDenseMaskEmbedHeadGTMask`) and, optionally, `embed`: a
    callable [B,N,C] -> [B,N,C'] for the detector's `embed_fcs` + `fc_embed` (:429-437)."""

    def __init__(self, num_proposals, track_head, embed=None):
        if track_head is None or not hasattr(track_head, 'match_loss_rows'):
            raise ValueError('TrackTrainTail needs the detector\'s track_head (QuasiDenseMaskEmbedHeadGTMask)')
        self.num_proposals, self.track_head, self.embed = int(num_proposals), track_head, embed

    def _rows(self, feats):
        feats = feats.reshape(feats.shape[0], feats.shape[1], -1)[:, :self.num_proposals]
        if self.embed is not None:
            feats = self.embed(feats)
        B, N = feats.shape[:2]
        return self.track_head(feats.reshape(B * N, -1)).reshape(B, N, -1)

    def _gt(self, assign_results):
        return torch.stack([(a.gt_inds if hasattr(a, 'gt_inds') else a)[:self.num_proposals].to(torch.int64) for a in assign_results])

    def __call__(self, object_feats_track, ref_obj_feats, key_assign_results, ref_assign_results, gt_match_indices):
        """object_feats_track, ref_obj_feats [B,N,C(,1,1)]: the head's tracking features of the key and the reference frames;
        key_assign_results, ref_assign_results: per image the `AssignResult` of `track_roi_assigner.assign` (:407-418; its `gt_inds`
        [>= num_proposals] is what is read) or that tensor itself; gt_match_indices: per image the int64 partner of every key-frame
        instance in the reference frame, -1 for none.  -> dict(loss_track[, loss_track_aux]) of `track_head.loss` (:454-460), under
        autograd.  Every image needs an assigned row in both frames (the reference asserts in its L2Loss otherwise)."""
        if not (torch.is_tensor(object_feats_track) and object_feats_track.is_cuda and ref_obj_feats.is_cuda):
            raise _lib.VknLibraryError('TrackTrainTail: expected CUDA/HIP tensors — the MI355X path has no CPU fallback')
        return self.track_head.match_loss_rows(self._rows(object_feats_track), self._rows(ref_obj_feats), self._gt(key_assign_results),
                                               self._gt(ref_assign_results), gt_match_indices)
