from .losses import batch_all_triplet_loss, batch_hard_triplet_loss

__all__ = ['batch_hard_triplet_loss', 'batch_all_triplet_loss']
