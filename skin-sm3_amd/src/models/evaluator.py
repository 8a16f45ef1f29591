"""Evaluators -- mirrors reference src/models/evaluator.py: the weighted kNN classifier `KNNOnlineEvaluator` (:11-120) on
the HIP engine (sm3hip/knn.py) and the linear-probe heads `LogisticRegressMultiHeadEvaluator` (:135-147)."""
import torch
import torch.nn as nn


class KNNOnlineEvaluator(nn.Module):
    """Weighted kNN classifier of Wu et al. 2018 (sec. 3.4): a query's class scores are the sums of exp(s / T) over its k
    most similar bank features of each class.  The similarity GEMM, the top-k and the vote run as HIP kernels
    (sm3hip.knn.knn_scores); GPU tensors only."""

    def __init__(self, train_dataloader, val_dataloader, n_classes, k=200, temperature=0.07) -> None:
        super().__init__()
        self.train_dataloader = train_dataloader
        self.val_dataloader = val_dataloader
        self.num_classes = n_classes
        self.k = k
        self.temperature = temperature

    def predict(self, query_feature, feature_bank, target_bank):
        """query_feature [B, D], feature_bank [N, D], target_bank [N] -> [B, C] class indices, best first (equal scores:
        lower class first)."""
        from sm3hip.knn import knn_scores
        (scores,) = knn_scores(query_feature, feature_bank, target_bank, self.num_classes, self.k, self.temperature)
        return scores.argsort(dim=-1, descending=True, stable=True)

    def predict_multilabel(self, query_feature, feature_bank, targets, num_classes):
        """targets [N, L], num_classes L ints -> the L vote tensors [B, C_l] (derm7pt: 8 labels)."""
        from sm3hip.knn import knn_scores
        return knn_scores(query_feature, feature_bank, targets, num_classes, self.k, self.temperature)

    @torch.no_grad()  # the reference's inference_mode: no_grad keeps the encoders' cached device buffers ordinary tensors
    def on_validation_epoch_end(self, model):
        """Bank from model(x).flatten(1) of the train loader (rows normalised), top-1 accuracy of the val loader's queries."""
        from sm3hip.knn import KNNBank, knn_scores, normalize
        model.eval()
        feature_bank, target_bank = [], []
        for inputs, labels in self.train_dataloader:
            x = inputs.cuda(non_blocking=True)
            feature_bank.append(normalize(model(x).flatten(start_dim=1)))
            target_bank.append(labels.cuda(non_blocking=True))
        bank = KNNBank(torch.cat(feature_bank, dim=0), torch.cat(target_bank, dim=0), self.num_classes)
        total_top1, total_num = 0.0, 0
        for inputs, labels in self.val_dataloader:
            x = inputs.cuda(non_blocking=True)
            target = labels.cuda(non_blocking=True)
            feature = normalize(model(x).flatten(start_dim=1))
            (scores,) = knn_scores(feature, bank, k=self.k, temperature=self.temperature)
            pred_labels = scores.argsort(dim=-1, descending=True, stable=True)
            total_num += x.shape[0]
            total_top1 += (pred_labels[:, 0] == target).float().sum().item()
        return total_top1 / total_num


class LogisticRegressMultiHeadEvaluator(nn.Module):
    def __init__(self, feat_dim, n_classes_per_label):
        super().__init__()
        self.classifier = nn.ModuleList([nn.Linear(feat_dim, i) for i in n_classes_per_label])
        for head in self.classifier:
            head.weight.data.normal_(mean=0.0, std=0.01)
            head.bias.data.zero_()

    def forward(self, x):
        return [classify(x) for classify in self.classifier]
