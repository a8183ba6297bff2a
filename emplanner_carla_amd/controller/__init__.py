"""Drop-in for the reference's ``controller`` package (controller/controller.py): Lateral_MPC_controller (:65-337),
Lateral_LQR_controller (:374-611), Longitudinal_PID_controller (:614-678), Vehicle_control (:680-724) and
Lateral_MPC__with_feedforward_controller (:727-990).

    from emplanner_carla_amd.controller.controller import Vehicle_control

Same constructors, public attributes and methods as the reference classes; the vehicle object is duck-typed (anything with
CARLA's ``get_location / get_transform / get_velocity / get_angular_velocity``), the controller arithmetic runs in the HIP
kernels behind ``emp_mpc_lateral`` / ``emp_lqr_lateral`` / ``emp_pid_longitudinal`` / ``emp_mpc_ff_lateral``, and
``Vehicle_control.run_step`` is one ``emp_vehicle_control`` launch (lateral law, PID and actuation).  Neither ``cvxopt`` nor
``carla`` is needed: without ``carla``, ``run_step`` returns a record with carla.VehicleControl's attributes.  INTEGRATION.md
shows the ``sys.modules`` swap that makes a driver's ``from controller.controller import Vehicle_control`` resolve here.
"""
from . import controller  # noqa: F401
