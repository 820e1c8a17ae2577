"""CCMatchInfo: a candidate match between connected components of two keyframes -- the CCs of frame 1 and of frame 2 that
overlap each other, directly or through a chain (AccessMath/evaluation/cc_match_info.py).  Same attributes and Merge as the release.

An addition: `pair_ink`, set by the overlay's Evaluator where it built the group from device counts -- (disp_y, disp_x, shared ink
pixels of all frame-1 / frame-2 pairs of the group under that displacement).  Evaluator.match_overlapping_ccs reads it, so the
four threshold pairs of a report launch nothing after the first."""


class CCMatchInfo:
    def __init__(self, matches1=None, matches2=None):
        self.frame1_ccs_refs = self._as_list(matches1)
        self.frame2_ccs_refs = self._as_list(matches2)
        self.pair_ink = None

    @staticmethod
    def _as_list(refs):
        if refs is None:
            return []
        return list(refs) if isinstance(refs, list) else [refs]

    @staticmethod
    def Merge(match1, match2):
        side1 = list(set(match1.frame1_ccs_refs) | set(match2.frame1_ccs_refs))
        side2 = list(set(match1.frame2_ccs_refs) | set(match2.frame2_ccs_refs))
        return CCMatchInfo(side1, side2)
