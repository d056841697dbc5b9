"""One table-coverage case of tests/test_gpu_rule.py on POISONED buffers
(LIFE_POISON=1, the fixture of tests/test_gpu_poison.py): every shard buffer
starts as 0xA5 -- live cells in the pitch padding, the aprons and the slack
rows.  The table-rule kernels rely, as the B3/S23 ones do, on never reading
those into a stored cell; under Day & Night a live neighbourhood breeds."""
import pytest

import rule_ref as R
from test_gpu_poison import poison  # noqa: F401
from test_gpu_rule import check_table

pytestmark = pytest.mark.gpu


def test_table_coverage_on_poison(gpu):
    check_table(gpu, R.NAMED["B3678/S34678"])
