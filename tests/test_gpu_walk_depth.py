"""The five sinks of k_walk — contribution records, weighted sums, attribute planes, attribute gradients, surface planes — on lists
beyond the 4096-word depth cache of the lazy order (tests/capacity_cases.py; contribution_reference.DEEP_CASES):

  single_tile_4097         one entry beyond the cache: the ninth selection orders a single streamed word
  four_deep_tiles          four tiles, every list deeper than the cache by more than a selection, walked to their ends
  ties_across_the_cache    tie groups of 700 / 65 / 64 clones across selection boundaries and the cache
  deep_list_ending_early   8193 entries, the walk ends at 4727: `range.y = range.x + min(..., tile_walked[tile])` cuts the walk's
                           list where the forward stopped ordering it; behind it ordered_ids holds padding

The walk reads the forward's ordered ids and traversal depths; the one-view tests of the sinks stop at a list of 1025 entries.  Every
case here goes through THEIR assertions (the functions of tests/test_gpu_contribution.py, test_gpu_weighted_contribution.py,
test_gpu_attributes.py, test_gpu_attribute_gradient.py and test_gpu_surface.py are called with the case's name), the exact ones
included: sum(pixels) == sum(hit counts), untouched records of unwalked rows, the adjoint identities, level mode against the
forward's alpha, largest-weight mode against the contribution records.  The CPU references are built once per case
(contribution_reference.case and the modules on top of it cache by name; tests/test_cpu_capacity_cases.py asserts their preconditions)."""
import pytest

from tests import contribution_reference as cr
from tests import test_gpu_attribute_gradient as t_attribute_gradient
from tests import test_gpu_attributes as t_attributes
from tests import test_gpu_contribution as t_contribution
from tests import test_gpu_surface as t_surface
from tests import test_gpu_weighted_contribution as t_weighted

pytestmark = pytest.mark.gpu

MAX_NEAR = cr.DEEP_MAX_NEAR      # the share of near pixels the surface references of these cases have: a property of the reference


@pytest.mark.parametrize("name", cr.DEEP_CASES)
def test_contribution_walk_on_deep_lists(name):
    t_contribution.test_scores_of_one_view(name)


@pytest.mark.parametrize("name", cr.DEEP_CASES)
def test_weighted_contribution_walk_on_deep_lists(name):
    t_weighted.test_weighted_scores_of_one_view(name)
    t_weighted.test_exact_identities(name)


@pytest.mark.parametrize("name", cr.DEEP_CASES)
def test_attribute_walk_on_deep_lists(name):
    t_attributes.test_planes_against_the_oracle(name)
    t_attributes.test_planes_against_the_devices_own_forward(name)
    t_attributes.test_adjoint_of_the_weighted_contribution_walk(name)
    t_attributes.test_exact_properties(name)


@pytest.mark.parametrize("name", cr.DEEP_CASES)
def test_attribute_gradient_walk_on_deep_lists(name):
    t_attribute_gradient.test_rows_against_the_reference(name)
    t_attribute_gradient.test_against_the_clamped_walk(name)
    t_attribute_gradient.test_adjoint_of_the_attribute_walk(name)
    t_attribute_gradient.test_exact_identities(name)


@pytest.mark.parametrize("name", cr.DEEP_CASES)
def test_surface_walk_on_deep_lists(name):
    t_surface.test_planes_against_the_reference(name, max_near=MAX_NEAR[name])
    t_surface.test_level_mode_against_the_forwards_alpha(name)
    t_surface.test_largest_weight_mode_against_the_contribution_records(name)
    t_surface.test_exact_properties(name)
