"""Sdf2SdfVisualizer (reference rigid_opt/sdf_2_sdf_visualizer.py): accepts the reference's parameters and draws
nothing -- this package writes no images or videos, like its other visualizer hooks."""


class Sdf2SdfVisualizer:
    class Parameters:
        def __init__(self, out_path="output/sdf_2_sdf_optimizer/", view_scaling_factor=8,
                     show_live_progression=False,
                     save_live_progression=False,
                     save_initial_fields=False,
                     save_final_fields=False,
                     save_warp_field_progression=False,
                     save_data_gradients=False):
            self.out_path = out_path
            self.view_scaling_factor = view_scaling_factor
            self.show_live_progress = show_live_progression
            self.save_live_field_progression = save_live_progression
            self.save_initial_fields = save_initial_fields
            self.save_final_fields = save_final_fields
            self.save_warp_field_progression = save_warp_field_progression
            self.save_data_gradients = save_data_gradients
            self.using_output_folder = (save_final_fields or save_initial_fields or save_live_progression or
                                        save_warp_field_progression or save_data_gradients)

    def __init__(self, parameters=None, field_size=128, level_count=4):
        self.field_size = field_size
        self.parameters = parameters if parameters else Sdf2SdfVisualizer.Parameters()
        self.level_count = level_count

    def generate_pre_optimization_visualizations(self, canonical_field, live_field):
        pass

    def generate_post_optimization_visualizations(self, canonical_field, live_field):
        pass

    def generate_per_iteration_visualizations(self, live_field):
        pass
