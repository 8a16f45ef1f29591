"""Per-label projectors of the multi-label heads -- the reference's src/models/projector.py surface, same modules, same
state_dict keys and shapes.  tools/mlc_train.py and tools/mlc_eval.py pick one with --mlc-proj (mlc_train.py:352-361):
v0 is nn.Identity (one label token, the features themselves), v1 / v2 / v3 are per-label BN-MLPs (bias-free Linear ->
BatchNorm1d -> ReLU, repeated, ending in BatchNorm1d(affine=False); projector.py:5-62), v4 is one biased Linear per label
(projector.py:65-78, what run.sh:39-56 trains with).  The native head path, sm3hip/mlc.py, runs all five on the HIP kernels;
these modules only hold the parameters and BatchNorm buffers (their forward is stock PyTorch, for reference use)."""
import torch.nn as nn


class _PerLabel(nn.Module):
    def __init__(self, in_dim, proj_dim, num_labels):
        super().__init__()
        self.projectors = nn.ModuleList([self._make_projector(in_dim, proj_dim) for _ in range(num_labels)])

    def forward(self, x):
        return [projector(x) for projector in self.projectors]


class MultiLabelProjector(_PerLabel):
    """v1: two in_dim-wide hidden layers per label."""

    def _make_projector(self, in_dim, proj_dim):
        return nn.Sequential(
            nn.Linear(in_dim, in_dim, bias=False), nn.BatchNorm1d(in_dim), nn.ReLU(inplace=True),
            nn.Linear(in_dim, in_dim, bias=False), nn.BatchNorm1d(in_dim), nn.ReLU(inplace=True),
            nn.Linear(in_dim, proj_dim, bias=False), nn.BatchNorm1d(proj_dim, affine=False),
        )


class MultiLabelProjector2(_PerLabel):
    """v2: one in_dim-wide hidden layer per label."""

    def _make_projector(self, in_dim, proj_dim):
        return nn.Sequential(
            nn.Linear(in_dim, in_dim, bias=False), nn.BatchNorm1d(in_dim), nn.ReLU(inplace=True),
            nn.Linear(in_dim, proj_dim, bias=False), nn.BatchNorm1d(proj_dim, affine=False),
        )


class MultiLabelProjector3(_PerLabel):
    """v3: Linear + BatchNorm1d(affine=False) per label."""

    def _make_projector(self, in_dim, proj_dim):
        return nn.Sequential(
            nn.Linear(in_dim, proj_dim, bias=False), nn.BatchNorm1d(proj_dim, affine=False),
        )


class MultiLabelProjector4(_PerLabel):
    """v4: one biased Linear per label."""

    def _make_projector(self, in_dim, proj_dim):
        return nn.Sequential(nn.Linear(in_dim, proj_dim))


MLC_PROJ_KINDS = ("v0", "v1", "v2", "v3", "v4")


def build_mlc_projectors(kind, in_dim, proj_dim, num_labels):
    """mlc_train.py:352-361 / mlc_eval.py:344-353.  Unknown kinds and a v0 whose width is not in_dim (the reference's
    TransformerEncoderLayer would fail on the first batch) are rejected here, before anything runs."""
    if kind not in MLC_PROJ_KINDS:
        raise ValueError(f"--mlc-proj must be one of {', '.join(MLC_PROJ_KINDS)}, got {kind!r}")
    if kind == "v0":
        if proj_dim != in_dim:
            raise ValueError(f"--mlc-proj v0 feeds the features themselves to the label attention: --mlc-proj-dim must equal "
                             f"the feature width {in_dim}, got {proj_dim}")
        return nn.Identity()
    return {"v1": MultiLabelProjector, "v2": MultiLabelProjector2, "v3": MultiLabelProjector3,
            "v4": MultiLabelProjector4}[kind](in_dim, proj_dim, num_labels)
