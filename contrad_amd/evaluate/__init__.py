"""Counterpart of the reference's ``evaluate`` package (evaluate/__init__.py:20-38): running averages for the
linear-evaluation loop."""


class AverageMeter(object):
    """Last value, weighted sum, count and running average of a scalar."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.value = self.average = self.sum = self.count = 0

    def update(self, value, n=1):
        self.value = value
        self.sum += value * n
        self.count += n
        self.average = self.sum / self.count
