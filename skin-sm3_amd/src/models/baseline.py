"""Dual-backbone linear-probe / fine-tune model on the HIP encoders -- drop-in for the reference's
`src/models/baseline.py:60-117` (`Baseline`), the model of `tools/backbone_eval.py`.

Two ResNet encoders (fc = Identity) run on sm3hip; under `--finetune fc` they are frozen and in eval mode, where
every conv + BatchNorm (+residual) (+ReLU) is ONE kernel (sm3_conv_bn_act_eval).  The eight classification
heads (Linear(4096, n_i), 98 K MACs per sample) stay stock PyTorch, as SURVEY.md 2.1 #5 scopes them.
`SingleBaseline` / `BaselineMLP1-3` of the reference file have no caller and are not provided; timm backbones
are not on the SM3 path.
"""
import torch
import torch.nn as nn

from .resnet import resnet18, resnet34, resnet50, resnet101, resnet152

NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]  # DIAG, PN, BWV, VS, PIG, STR, DaG, RS (backbone_eval.py:60-62)


_REFERENCE_DEFAULT = object()


class Baseline(nn.Module):
    def __init__(self, arch="resnet50", weights=_REFERENCE_DEFAULT):
        """weights: None (random initialisation), a state_dict path, or a torchvision enum name served from the local
        torch-hub cache (src/models/resnet.py).  Left out, it is None for the Bottleneck archs -- this mirror's default
        since it was built -- and, for the BasicBlock archs, the reference's own default (baseline.py:61,
        weights="IMAGENET1K_V1"): Baseline("resnet18") means ImageNet-pretrained encoders there, and without the cached
        file that raises NotImplementedError here instead of silently training from random weights.
        tools/backbone_eval.py always passes weights explicitly (--arch-weights, default None)."""
        super().__init__()
        ctor = {"resnet18": resnet18, "resnet34": resnet34, "resnet50": resnet50, "resnet101": resnet101,
                "resnet152": resnet152}.get(arch)
        if ctor is None:
            raise NotImplementedError(f"arch {arch!r}: the SM3 HIP engine implements the torchvision ResNets")
        if weights is _REFERENCE_DEFAULT:
            weights = "IMAGENET1K_V1" if arch in ("resnet18", "resnet34") else None
        self.derm_backbone = ctor(weights=weights)
        self.clinic_backbone = ctor(weights=weights)
        feat_dim = self.derm_backbone.fc.in_features * 2  # 512 * 2 (resnet18/34) or 2048 * 2
        self.derm_backbone.fc = nn.Identity()
        self.clinic_backbone.fc = nn.Identity()
        self.classifier = nn.ModuleList([nn.Linear(feat_dim, n) for n in NUM_CLASSES])
        for layer in self.classifier:
            layer.weight.data.normal_(mean=0.0, std=0.01)
            layer.bias.data.zero_()

    def forward(self, x):
        derm_feats = self.derm_backbone(x[0])
        clinic_feats = self.clinic_backbone(x[1])
        feats = torch.cat([derm_feats, clinic_feats], dim=1)
        return [classify(feats) for classify in self.classifier]

    def freeze_backbone(self):
        for p in list(self.derm_backbone.parameters()) + list(self.clinic_backbone.parameters()):
            p.requires_grad = False

    def unfreeze_backbone(self):
        for p in list(self.derm_backbone.parameters()) + list(self.clinic_backbone.parameters()):
            p.requires_grad = True
