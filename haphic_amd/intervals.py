"""The slice of the `portion` package that scripts/HapHiC_refsort.py uses (:72-73, :229), for boxes where it is not installed and
`python -m haphic_amd refsort --stub-missing-imports` is given: closed intervals of numbers with `&`, `.empty`, `.lower`, `.upper` and `in`.
The device path never builds one; the reference's own functions do when a call is handed back to them."""


class Closed:
    __slots__ = ('lower', 'upper')

    def __init__(self, lower, upper):
        self.lower, self.upper = lower, upper

    @property
    def empty(self):
        return self.lower > self.upper

    def __and__(self, other):
        if self.empty or other.empty:
            return Closed(1, 0)
        return Closed(max(self.lower, other.lower), min(self.upper, other.upper))

    def __contains__(self, x):
        return self.lower <= x <= self.upper

    def __repr__(self):
        return '()' if self.empty else '[{},{}]'.format(self.lower, self.upper)


def closed(lower, upper):
    return Closed(lower, upper)
